// strsim_extract.h -- top-k search by Indel similarity with a score cutoff (strsim_extract_device): for
// every query, the k candidates with the highest score >= score_cutoff, score = indel(q, c) = 1.0 - d / (|q| + |c|)
// (epilogue_indel of strsim_indel.h; rapidfuzz's process.extract with fuzz.ratio / 100).
//
// This header holds what the host shares with the kernel (tests/cpu_harness/extract_harness.cpp compiles it with g++): the rank
// table that orders scores without a division per pair, the window / skip / stop rules of a wave's sweep and the Indel core on
// wave-uniform text, and ExtractRules, which hands them to the one sweep loop that nearest match runs too (search_sweep_lane of
// strsim_nearest_kernels.h on the device, tests/cpu_harness/sweep_host.h on the host).  The kernel is in
// strsim_extract_kernels.h.
//
// Ranking.  In the lane class both strings have at most 32 bytes, so a pair is (d, s) with s = |q| + |c| <= 64 and d <= s.  Two
// distinct rationals d / s with s <= 64 differ by at least 1 / (64 * 63), far more than an ulp, so the correctly rounded f64
// quotient and then 1.0 - quotient order them strictly, and equal rationals give equal doubles: the f64 score orders pairs
// exactly as d / s does.  The host therefore sorts the distinct scores once (rank 0 = 1.0, the best) and a pair's score is
// looked up as rank[s][d]; a list holds keys rank << 32 | j, ascending = match_better's order (descending score, ties to the
// lower candidate index), and the f64 score of a kept entry is epilogue_indel of its rank's representative (d, s).  A cutoff
// becomes `rlimit`, the number of ranks whose score is >= score_cutoff: rank r is admissible iff r < rlimit.
//
// The sweep of one wave (64 queries of the lane class, taken in length order, lengths lmin..lmax).  d >= ||q| - |c||, so no
// candidate of length lc scores above ub(lq, lc) = E(|lq - lc|, lq + lc), looked up in the same table (never a separately
// rounded expression).  For a fixed lq, (|lq - lc|) / (lq + lc) grows strictly as lc moves away from lq on either side (for
// lq = 0 it is 1 for every lc > 0), so ub's rank never falls on the way out:
//   - static window: below lmin the query of length lmin has the highest ub ((lq - lc) / (lq + lc) grows with lq), above lmax
//     the one of length lmax; [lo, hi] are the lengths those two admit under the cutoff alone, and no query of the wave can
//     have an admissible candidate outside;
//   - the lengths inside it are visited nearest-first (nearest_step_range): step 0 is lmin..lmax, step g is lmin - g, lmax + g;
//   - skip: a lane's bound is the rank of its K-th entry once the list is full, else the last admissible rank; it needs
//     length lc iff rank(ub(lq, lc)) <= bound -- not strict, because a tie with a lower index still enters.  A candidate no
//     lane needs is skipped by the wave (a ballot); bounds only fall, so the rest of that length's slice goes with it;
//   - stop: when no live lane needs either length of step g, by the monotonicity above none needs any length of a later step.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "strsim_indel.h"
#include "strsim_nearest.h"

namespace strsim {

constexpr uint32_t EXTRACT_MAX_SUM = 2u * NEAREST_MAX_LEN;                    // s = lq + lc of a lane-class pair
constexpr uint32_t EXTRACT_TAB_W = EXTRACT_MAX_SUM + 1u;                      // row s of the table: d = 0..64
constexpr uint32_t EXTRACT_TAB_N = EXTRACT_TAB_W * EXTRACT_TAB_W;             // 4 225 entries
constexpr uint32_t EXTRACT_TAB_WORDS = (EXTRACT_TAB_N + 1u) / 2u;             // ... as 32-bit words (the LDS copy)
constexpr uint32_t EXTRACT_MAX_RANKS = 2048u;                                 // 1 + sum of phi(1..64) = 1 261 distinct scores
constexpr uint16_t EXTRACT_NO_RANK = 0xFFFFu;                                 // d > s: no such pair

struct ExtractTable {
    uint16_t rank[2u * EXTRACT_TAB_WORDS]; // rank[s * EXTRACT_TAB_W + d], 0 = the score 1.0
    uint16_t rep[EXTRACT_MAX_RANKS];       // a pair (d << 8 | s) of every rank
    uint32_t nranks, pad;
};

// The f64 score of rank r: the same two operations as every pairwise Indel score.
STRSIM_HD double extract_rank_score(const uint16_t *rep, uint32_t r) { return epilogue_indel(rep[r] >> 8, rep[r] & 0xFFu, 0u); }

// Host: every (d, s) with d <= s <= 64 sorted by its f64 score, descending; equal scores share a rank.
inline void extract_build_table(ExtractTable &t)
{
    struct Pair { double score; uint16_t ds; };
    Pair p[EXTRACT_TAB_N];
    uint32_t n = 0;
    for (uint32_t s = 0; s <= EXTRACT_MAX_SUM; ++s)
        for (uint32_t d = 0; d <= s; ++d) p[n++] = Pair{epilogue_indel(d, s, 0u), (uint16_t)(d << 8 | s)};
    std::stable_sort(p, p + n, [](const Pair &a, const Pair &b) { return a.score > b.score; });
    for (uint32_t x = 0; x < 2u * EXTRACT_TAB_WORDS; ++x) t.rank[x] = EXTRACT_NO_RANK;
    for (uint32_t x = 0; x < EXTRACT_MAX_RANKS; ++x) t.rep[x] = 0u;
    uint32_t r = 0;
    for (uint32_t x = 0; x < n; ++x) {
        if (x && p[x].score != p[x - 1].score) ++r;
        if (x == 0 || p[x].score != p[x - 1].score) t.rep[r] = p[x].ds;
        t.rank[(p[x].ds & 0xFFu) * EXTRACT_TAB_W + (p[x].ds >> 8)] = (uint16_t)r;
    }
    t.nranks = r + 1u;
    t.pad = 0u;
}

// Host: the number of ranks whose score is >= cutoff (0: nothing is admissible; nranks: everything).  cutoff is not NaN.
inline uint32_t extract_rank_limit(const ExtractTable &t, double cutoff)
{
    uint32_t lo = 0, hi = t.nranks; // scores fall with the rank: the first rank whose score is < cutoff
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
        if (extract_rank_score(t.rep, mid) >= cutoff) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// The rank of a pair with distance d and length sum s (d <= s <= 64).
STRSIM_HD uint32_t extract_rank(const uint16_t *rank, uint32_t d, uint32_t s) { return rank[s * EXTRACT_TAB_W + d]; }

// The rank of ub(lq, lc), the best score a candidate of length lc can reach against a query of length lq.
STRSIM_HD uint32_t extract_ub(const uint16_t *rank, uint32_t lq, uint32_t lc) { return extract_rank(rank, lq > lc ? lq - lc : lc - lq, lq + lc); }

// A list entry (rank, j) as one key: ascending keys are descending scores, ties to the lower candidate index j.
STRSIM_HD uint64_t extract_key(uint32_t r, uint32_t j) { return ((uint64_t)r << 32) | j; }

// The bound of a lane: the rank of its K-th entry, or the last admissible rank while the list is not full (an empty K-th slot
// has rank 0xFFFFFFFF).  rlimit >= 1.
STRSIM_HD uint32_t extract_bound(uint64_t kth, uint32_t rlimit)
{
    const uint32_t r = (uint32_t)(kth >> 32);
    return r < rlimit - 1u ? r : rlimit - 1u;
}

// Whether a lane with bound b needs a length whose ub has rank ubr: a pair that ties the bound may still enter.
STRSIM_HD bool extract_needs(uint32_t ubr, uint32_t b) { return ubr <= b; }

// Static window of a wave whose live queries have lengths lmin..lmax under rlimit >= 1: candidate lengths [lo, hi].  ub falls
// monotonically on the way out, so each side ends at the first length that is not admissible.
STRSIM_HD void extract_window(const uint16_t *rank, uint32_t lmin, uint32_t lmax, uint32_t rlimit, uint32_t &lo, uint32_t &hi)
{
    lo = lmin;
    while (lo > 0u && extract_ub(rank, lmin, lo - 1u) < rlimit) --lo;
    hi = lmax;
    while (hi < NEAREST_MAX_LEN && extract_ub(rank, lmax, hi + 1u) < rlimit) ++hi;
}

// Indel distance of a pattern of lp <= 32 ASCII bytes (NP bit-planes, build_planes) against a text of lt <= 32 bytes in wt: the
// step of strsim_indel.h on one 32-bit word.  Rows at and above lp are masked out of the popcount; they hold the zero padding
// of the pattern, which a NUL byte of the text matches, but the carry of the add only travels upward, so they cannot change
// a counted row -- a NUL byte is a legal character on either side.  lp = 0 counts no rows (d = lt), lt = 0 runs no column.
template <int NP>
STRSIM_HD uint32_t extract_indel_uniform_text(const uint32_t (&wt)[8], uint32_t lt, const uint32_t (&P)[NP], uint32_t lp)
{
    uint32_t V = 0xFFFFFFFFu;
    for (uint32_t w = 0; w < (lt + 3u) / 4u; ++w) unrolled_until<0, 4>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if (4u * w + (uint32_t)b >= lt) return false;
        const uint32_t Eq = eq_mask<NP>(P, 0xFFFFFFFFu, wt[w], b);
        const uint32_t u = V & Eq;
        V = (V + u) | (V & ~Eq);
        return true;
    });
    const uint32_t l = popc32(~V & low_ones(lp));
    return lp + lt - 2u * l;
}

// The rule set of the extract sweep over a rank table (`rank`: the kernel's LDS copy) under rlimit >= 1.  The value a lane
// keeps per candidate length is the rank of ub(lq, lc) and the table row of the pair's length sum, so a pair costs one read;
// the sweep stops after a step none of whose lengths any live lane needed.
struct ExtractRules {
    static constexpr bool STOP_BY_BOUND = false;
    struct Len { uint32_t ubr; const uint16_t *row; };
    const uint16_t *rank, *rep;
    uint32_t rlimit;
    STRSIM_HD void window(uint32_t lmin, uint32_t lmax, uint32_t &lo, uint32_t &hi) const { extract_window(rank, lmin, lmax, rlimit, lo, hi); }
    STRSIM_HD Len at(uint32_t lq, uint32_t lc) const { return Len{extract_ub(rank, lq, lc), rank + (lq + lc) * EXTRACT_TAB_W}; }
    STRSIM_HD bool needs(uint32_t, const Len &len, uint64_t kth) const { return extract_needs(len.ubr, extract_bound(kth, rlimit)); }
    template <int NP>
    STRSIM_HD uint32_t distance(const uint32_t (&wt)[8], uint32_t lc, const uint32_t (&P)[NP], uint32_t lq) const
    {
        return extract_indel_uniform_text<NP>(wt, lc, P, lq);
    }
    STRSIM_HD uint64_t key(uint32_t d, const Len &len, uint32_t j, bool &ok) const
    {
        const uint32_t r = len.row[d]; // d <= lq + lc: inside the row
        ok = r < rlimit;
        return extract_key(r, j);
    }
    STRSIM_HD double score(uint64_t key) const { return extract_rank_score(rep, (uint32_t)(key >> 32)); }
};

} // namespace strsim
