// strsim_nearest.h -- nearest-match search by bounded edit distance (strsim_nearest_device): for every
// query, the k candidates with the smallest d <= max_distance, d the Levenshtein (measure 0) or OSA (measure 6) distance.
//
// This header holds what the host shares with the kernels (tests/cpu_harness/nearest_harness.cpp compiles it with g++): the
// order of a list, the window / skip / stop rules of a wave's sweep and the two distance cores on wave-uniform text, and
// NearestRules, which hands them to the one sweep loop (search_sweep_lane of strsim_nearest_kernels.h on the device,
// tests/cpu_harness/sweep_host.h on the host; strsim_extract.h has the other rule set).  The kernels are in
// strsim_nearest_kernels.h.
//
// The sweep of one wave (64 queries of the lane class, taken in length order, so they span one or two lengths lmin..lmax):
//   - static window: candidate lengths outside [lmin - kmax, lmax + kmax] are never visited (d >= | |a| - |b| | > kmax);
//   - the lengths inside it are visited nearest-first: step 0 is lmin..lmax, step g >= 1 is lmin - g and lmax + g;
//   - skip: a lane whose list is full has the bound b = min(kmax, its K-th distance), else b = kmax; it needs a candidate of
//     length lc only when |lq - lc| <= b (a candidate that ties the K-th distance with a lower index still enters, so the
//     comparison is strict the other way round).  A candidate no lane needs is skipped by the wave (a ballot); bounds only
//     shrink, so the rest of that length is skipped with it;
//   - stop: every length of step g is at least g away from every query length, so once g exceeds the largest bound of the
//     wave's live lanes nothing that remains can enter any list.
#pragma once
#include <stdint.h>

#include "strsim_osa.h"

namespace strsim {

constexpr uint32_t NEAREST_MAX_LEN = 32u;        // the lane class of k_match_pack: ASCII strings of at most 32 bytes
constexpr uint32_t NEAREST_SLOW_BUCKET = 33u;    // length buckets 0..32, then the slow strings (queries only)
constexpr uint32_t NEAREST_BUCKETS = 34u;
constexpr uint64_t NEAREST_EMPTY = ~0ull;        // an empty slot: distance and index 0xFFFFFFFF

// A list entry (d, j) as one key: ascending keys are ascending d, ties to the lower candidate index j.
STRSIM_HD uint64_t nearest_key(uint32_t d, uint32_t j) { return ((uint64_t)d << 32) | j; }

// Static window of a wave whose live queries have lengths lmin..lmax: candidate lengths [lo, hi].
STRSIM_HD void nearest_window(uint32_t lmin, uint32_t lmax, uint32_t kmax, uint32_t &lo, uint32_t &hi)
{
    lo = lmin > kmax ? lmin - kmax : 0u;
    hi = kmax < NEAREST_MAX_LEN - lmax ? lmax + kmax : NEAREST_MAX_LEN;
}

// Steps of the nearest-first order inside the window: step 0 and then one per length of distance g on either side.
STRSIM_HD uint32_t nearest_steps(uint32_t lmin, uint32_t lmax, uint32_t lo, uint32_t hi)
{
    const uint32_t below = lmin - lo, above = hi - lmax;
    return 1u + (below > above ? below : above);
}

// The candidate lengths of step g as first, first + stride, ..., last: lmin..lmax for g = 0, else lmin - g and lmax + g, each
// only if it lies inside the window [lo, hi].  False when step g has no length in the window.
STRSIM_HD bool nearest_step_range(uint32_t lmin, uint32_t lmax, uint32_t lo, uint32_t hi, uint32_t g, uint32_t &first,
                                  uint32_t &last, uint32_t &stride)
{
    if (g == 0u) {
        first = lmin; last = lmax; stride = 1u;
        return true;
    }
    const bool down = lmin >= lo + g, up = lmax + g <= hi;
    first = down ? lmin - g : lmax + g;
    last = up ? lmax + g : lmin - g;
    stride = lmax - lmin + 2u * g;
    return down || up;
}

// The bound of a lane: min(kmax, the distance of its K-th entry); an empty K-th slot has distance 0xFFFFFFFF, so it is kmax.
STRSIM_HD uint32_t nearest_bound(uint64_t kth, uint32_t kmax)
{
    const uint32_t d = (uint32_t)(kth >> 32);
    return d < kmax ? d : kmax;
}

// Whether a query of length lq with bound b needs a candidate of length lc: d >= |lq - lc|, and d = b may still enter.
STRSIM_HD bool nearest_needs(uint32_t lq, uint32_t lc, uint32_t b) { return (lq > lc ? lq - lc : lc - lq) <= b; }

// Whether the sweep is over before step `next`: every length left is at least `next` away from every query length.
STRSIM_HD bool nearest_done(uint32_t next, uint32_t max_bound) { return next > max_bound; }

// (key) into a sorted list of K keys: one compare-and-swap per slot, fully unrolled (the slots stay in registers)
template <int K>
STRSIM_HD void nearest_insert(uint64_t (&keys)[K], uint64_t v)
{
#pragma unroll
    for (int s = 0; s < K; ++s) {
        const uint64_t t = keys[s];
        const bool sw = v < t;
        keys[s] = sw ? v : t;
        v = sw ? t : v;
    }
}

// Levenshtein distance of a pattern of lp <= 32 ASCII bytes (NP bit-planes, build_planes) against a text of lt <= 32 bytes in
// wt: the column of lit_lev_uniform_text (strsim_lane_lit.h), one column per step instead of pairs of columns -- the paired form
// runs out of scalar registers in k_nearest_lane, whose sweep keeps more of them live.  lp = 0 counts no rows (d = lt), lt = 0
// runs no column (d = lp).
template <int NP>
STRSIM_HD uint32_t nearest_lev_uniform_text(const uint32_t (&wt)[8], uint32_t lt, const uint32_t (&P)[NP], uint32_t lp)
{
    uint32_t Pv = 0xFFFFFFFFu, Mv = 0u;
    for (uint32_t w = 0; w < (lt + 3u) / 4u; ++w) unrolled_until<0, 4>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if (4u * w + (uint32_t)b >= lt) return false;
        const uint32_t Eq = eq_mask<NP>(P, 0xFFFFFFFFu, wt[w], b);
        const uint32_t D0 = bitop3<0xBE>((Eq & Pv) + Pv, Pv, Eq) | Mv; // (((Eq & Pv) + Pv) ^ Pv) | Eq | Mv
        const uint32_t nX = twice(bitop3<0x0E>(Mv, D0, Pv));          // ~((HP << 1) | 1)
        const uint32_t HN2 = twice(D0 & Pv);                           // HN << 1
        Pv = bitop3<0xF2>(HN2, D0, nX);                                // (HN << 1) | ~(D0 | X)
        Mv = bitop3<0x50>(D0, D0, nX);                                 // D0 & X
        return true;
    });
    const uint32_t rows = low_ones(lp);
    return lt + popc32(Pv & rows) - popc32(Mv & rows);
}

// OSA distance of a pattern of lp <= 32 ASCII bytes (NP bit-planes, build_planes) against a text of lt <= 32 bytes in wt: the
// step of strsim_osa.h on 32-bit masks.  On the device the text is wave-uniform, so lt and the bit fills of wt are scalar.  An
// empty side needs no special case: lp = 0 counts no rows (d = lt), lt = 0 runs no column (d = lp).
template <int NP>
STRSIM_HD uint32_t nearest_osa_uniform_text(const uint32_t (&wt)[8], uint32_t lt, const uint32_t (&P)[NP], uint32_t lp)
{
    uint32_t VP = 0xFFFFFFFFu, VN = 0u, D0p = 0u, EQp = 0u;
    for (uint32_t w = 0; w < (lt + 3u) / 4u; ++w) unrolled_until<0, 4>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if (4u * w + (uint32_t)b >= lt) return false;
        osa_step<uint32_t>(eq_mask<NP>(P, 0xFFFFFFFFu, wt[w], b), VP, VN, D0p, EQp);
        return true;
    });
    const uint32_t rows = low_ones(lp);
    return lt + popc32(VP & rows) - popc32(VN & rows);
}

// The rule set of the nearest-match sweep (TR: OSA instead of Levenshtein).  The value a lane keeps per candidate length is
// the length itself; the sweep stops before step g once g exceeds the largest bound of the wave's live lanes.
template <bool TR>
struct NearestRules {
    static constexpr bool STOP_BY_BOUND = true;
    uint32_t kmax;
    STRSIM_HD void window(uint32_t lmin, uint32_t lmax, uint32_t &lo, uint32_t &hi) const { nearest_window(lmin, lmax, kmax, lo, hi); }
    STRSIM_HD uint32_t at(uint32_t, uint32_t lc) const { return lc; }
    STRSIM_HD uint32_t bound(uint64_t kth) const { return nearest_bound(kth, kmax); }
    STRSIM_HD bool needs(uint32_t lq, uint32_t lc, uint64_t kth) const { return nearest_needs(lq, lc, bound(kth)); }
    STRSIM_HD bool done(uint32_t next, uint32_t max_bound) const { return nearest_done(next, max_bound); }
    template <int NP>
    STRSIM_HD uint32_t distance(const uint32_t (&wt)[8], uint32_t lc, const uint32_t (&P)[NP], uint32_t lq) const
    {
        return TR ? nearest_osa_uniform_text<NP>(wt, lc, P, lq) : nearest_lev_uniform_text<NP>(wt, lc, P, lq);
    }
    STRSIM_HD uint64_t key(uint32_t d, uint32_t, uint32_t j, bool &ok) const { ok = d <= kmax; return nearest_key(d, j); }
    STRSIM_HD double score(uint64_t key) const { return -(double)(uint32_t)(key >> 32); } // (match_better's order: ascending d)
};

} // namespace strsim
