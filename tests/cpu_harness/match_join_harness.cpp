// match_join_harness.cpp -- host build of the rules strsim_match_join.h shares with k_match_join_lane
// (strsim_match_join_kernels.h), for tests/test_match_join_cpu.py: g++ compiles the same headers.
//   mj_bound_check   for every pair of lengths 0 .. 32: the maximum of the measure's own epilogue over EVERY integer tuple the
//                    kernel can produce (d in |lq - lc| .. max; m <= min, t <= m, prefix <= min(4, min); isect <= min) against
//                    match_join_ub -- no tuple above the bound, and the bound attained.
//   mj_need_mask     the library's need mask of a call, for the comparison with match_join_ub >= cutoff made directly.
//   mj_replay        join_replay_host of join_sweep_host.h (a wave's count sweep, the counts -> prefix -> 64-bit scan, its fill sweep
//                    and the row sort against brute force, with every check of the protocol: the replay of join_harness.cpp) under
//                    k_match_join_lane's own part: the lanes' words of the need mask and the lengths whose bit is set, a pair
//                    yielding its f64 score, over a random score matrix that respects the bound; and, of its own, that the sweeps
//                    visit exactly the allowed lengths and that a clear bit of the mask loses no hit.
// Built as a shared library; with -DMATCH_JOIN_HARNESS_MAIN it is a stand-alone program that runs every case (the form that is run
// under the address and undefined-behaviour sanitizers).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <numeric>
#include <vector>

#include "join_sweep_host.h"
#include "strsim_match_join.h"

using namespace strsim;

// The integers a pair's score is made of; which of them a measure reads is the measure's business.
struct Tuple {
    uint32_t d, m, t, prefix, isect;
};

// The score of a pair of lengths (lq, lc) whose cores returned `u`: the library's epilogues, the empty strings as every kernel
// answers them (1.0 for two, 0.0 for one).
static double score_of(int measure, uint32_t lq, uint32_t lc, const Tuple &u)
{
    if (lq == 0u && lc == 0u) return 1.0;
    if (lq == 0u || lc == 0u) return 0.0;
    switch (measure) {
    case LEVENSHTEIN: return epilogue_levenshtein(u.d, lq, lc);
    case JARO: return epilogue_jaro(u.m, u.t, lq, lc);
    case JARO_WINKLER: return epilogue_jaro_winkler(epilogue_jaro(u.m, u.t, lq, lc), u.prefix);
    case JACCARD: return epilogue_jaccard(u.isect, lq, lc);
    default: return epilogue_sorensen_dice(u.isect, lq, lc);
    }
}

// f(tuple) for every tuple the kernel can produce at these lengths (only the integers `measure` reads are varied).
template <class F>
static void every_tuple(int measure, uint32_t lq, uint32_t lc, F f)
{
    const uint32_t mn = std::min(lq, lc), mx = std::max(lq, lc), pmax = std::min(4u, mn);
    Tuple u{mx - mn, 0u, 0u, 0u, 0u};
    if (measure == LEVENSHTEIN) {
        for (u.d = mx - mn; u.d <= mx; ++u.d) f(u);
    } else if (measure == JARO || measure == JARO_WINKLER) {
        for (u.m = 0; u.m <= mn; ++u.m)
            for (u.t = 0; u.t <= u.m; ++u.t)
                for (u.prefix = 0; u.prefix <= (measure == JARO_WINKLER ? pmax : 0u); ++u.prefix) f(u);
    } else {
        for (u.isect = 0; u.isect <= mn; ++u.isect) f(u);
    }
}

static Tuple random_tuple(Rng &g, uint32_t lq, uint32_t lc)
{
    const uint32_t mn = std::min(lq, lc), mx = std::max(lq, lc);
    Tuple u;
    // near pairs are common: most of the time within three of the best integers
    const bool near = g.below(3) != 0u;
    u.d = near ? std::min(mx, mx - mn + g.below(4)) : mx - mn + g.below(mn + 1);
    u.m = near ? mn - g.below(std::min(mn, 3u) + 1) : g.below(mn + 1);
    u.t = near ? g.below(std::min(u.m, 2u) + 1) : g.below(u.m + 1);
    u.prefix = g.below(std::min(4u, mn) + 1);
    u.isect = near ? mn - g.below(std::min(mn, 3u) + 1) : g.below(mn + 1);
    return u;
}

extern "C" double mj_ub(int measure, uint32_t lq, uint32_t lc) { return match_join_ub(measure, lq, lc); }

// 0, or how many length pairs have a tuple above the bound or none that attains it.
extern "C" uint32_t mj_bound_check(int measure)
{
    uint32_t bad = 0;
    for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq)
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
            const double ub = match_join_ub(measure, lq, lc);
            bool above = false, attained = false;
            every_tuple(measure, lq, lc, [&](const Tuple &u) {
                const double v = score_of(measure, lq, lc, u);
                if (!(v <= ub)) above = true; // (a NaN would count too)
                if (v == ub) attained = true;
            });
            if (above || !attained) ++bad;
        }
    return bad;
}

// The library's need mask of a call into out[33]; returns whether any bit is set.
extern "C" int mj_need_mask(int measure, double cutoff, uint64_t *out)
{
    MatchJoinNeed need;
    const bool any = match_join_need_mask(measure, cutoff, need);
    memcpy(out, need.w, sizeof need.w);
    return any ? 1 : 0;
}

extern "C" uint32_t mj_lengths(void) { return MATCH_JOIN_LENGTHS; }
extern "C" uint32_t mj_need_bytes(void) { return (uint32_t)sizeof(MatchJoinNeed); }

// What k_match_join_lane adds to the shared sweep, over given scores score[i * nc + j].
struct MaskCase {
    int measure;
    const std::vector<uint32_t> &qlen;
    const double *score;
    uint32_t nc;
    double cutoff;
    MatchJoinNeed need;
    bool nothing;
    uint64_t allowed, seen; // the lengths some query needs; the lengths the sweep in hand visited
    uint64_t *stats;

    double expected(uint32_t i, uint32_t j) const { return score[(size_t)i * nc + j]; }

    // k_match_join_lane's loop over the lengths: the lane's word of the mask and the wave's (the loop over the 33 words with a
    // uniform index), then exactly the lengths whose bit is set, in ascending order
    void lengths(JoinWave &W, bool fill, uint32_t split)
    {
        std::vector<uint64_t> mine(W.nq, 0);
        uint64_t wave = 0;
        for (uint32_t l = 0; l < MATCH_JOIN_LENGTHS; ++l) {
            const uint64_t w = need.w[l];
            bool any = false;
            for (uint32_t i = 0; i < W.nq; ++i)
                if (qlen[i] == l) { mine[i] = w; any = true; }
            if (any) wave |= w;
        }
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
            if (!((wave >> lc) & 1ull)) continue;
            seen |= 1ull << lc;
            join_slice_host(
                W, fill, split, lc, [&](uint32_t i) { return ((mine[i] >> lc) & 1ull) != 0ull; }, [&](uint32_t) { return MatchJoinRule{cutoff}; },
                [&](uint32_t i, uint32_t j) { return score[(size_t)i * nc + j]; });
        }
    }

    int after(const JoinWave &W, bool fill)
    {
        const uint64_t visited = seen;
        seen = 0;
        if (!fill) stats[2] = visited;
        if (visited != allowed) return 13; // exactly the lengths whose bit is set in some live lane's word
        if (fill) return 0;
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) // (and a clear bit is a true statement: no hit was lost to it)
            for (uint32_t i = 0; i < W.nq; ++i)
                if (!match_join_needs(need, qlen[i], lc) && match_join_ub(measure, qlen[i], lc) >= cutoff) return 14;
        return 0;
    }
};

// nq <= 64 queries and nc candidates of random lengths 0 .. maxlen, every pair's score the measure's epilogue of a random tuple;
// stats[0] = candidates visited by one sweep (out of nc), stats[1] = hits, stats[2] = the lengths the count sweep visited (bits).
// 0, or the number of the first check that failed.
extern "C" int mj_replay(uint64_t seed, int measure, uint32_t nq, uint32_t nc, uint32_t maxlen, double cutoff, int upper, uint32_t splits,
                         int undersize, uint32_t shift, uint64_t *stats)
{
    Rng g{seed * 2654435761ull + 12345u + (uint64_t)measure * 977u};
    std::vector<uint32_t> qlen(nq), clen(nc);
    std::vector<double> score((size_t)nq * nc);
    for (auto &l : qlen) l = g.below(maxlen + 1);
    for (auto &l : clen) l = g.below(maxlen + 1);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < nc; ++j) score[(size_t)i * nc + j] = score_of(measure, qlen[i], clen[j], random_tuple(g, qlen[i], clen[j]));
    stats[2] = 0;
    MaskCase C{measure, qlen, score.data(), nc, cutoff, {}, false, 0, 0, stats};
    C.nothing = !match_join_need_mask(measure, cutoff, C.need);
    // the lengths some query needs: the union the sweep may visit and nothing else
    for (uint32_t i = 0; i < nq; ++i) C.allowed |= C.need.w[qlen[i]];
    return join_replay_host(C, nq, clen, upper != 0, splits, undersize, shift, stats);
}

// The cutoffs of the suite for a measure: -inf, 0, 0.5, 0.8, 1.0, 1.5, and ub(measure, 7, 9) with its two f64 neighbours.
extern "C" uint32_t mj_cutoffs(int measure, double *out)
{
    const double e = match_join_ub(measure, 7, 9), inf = std::numeric_limits<double>::infinity();
    const double cuts[9] = {-inf, 0.0, 0.5, 0.8, 1.0, 1.5, nextafter(e, 0.0), e, nextafter(e, 2.0)};
    memcpy(out, cuts, sizeof cuts);
    return 9u;
}

// Every case of the sweep; the count of failures.
extern "C" uint32_t mj_replay_all(void)
{
    uint32_t failed = 0;
    uint64_t stats[3];
    double cuts[9];
    for (int measure = 0; measure < 5; ++measure) {
        const uint32_t ncuts = mj_cutoffs(measure, cuts);
        for (uint32_t c = 0; c < ncuts; ++c)
            for (int upper = 0; upper < 2; ++upper)
                for (uint32_t splits = 1; splits <= 3; ++splits)
                    for (uint32_t shift = 0; shift < 3; ++shift) // hit-map groups of 1, 2 and 4 positions
                        for (int under = 0; under < 2; ++under)
                            for (uint64_t seed = 0; seed < 4; ++seed) {
                                const uint32_t nq = seed == 0 ? 1u : seed == 1 ? 64u : 1u + (uint32_t)(seed * 11u);
                                const uint32_t nc = seed == 2 ? 0u : 40u + (uint32_t)seed * 37u;
                                if (mj_replay(seed + 100 * c, measure, nq, nc, seed == 3 ? 6u : 32u, cuts[c], upper, splits, under, shift, stats)) ++failed;
                            }
    }
    return failed;
}

#ifdef MATCH_JOIN_HARNESS_MAIN
int main()
{
    uint32_t bounds = 0, masks = 0;
    double cuts[9];
    for (int measure = 0; measure < 5; ++measure) {
        bounds += mj_bound_check(measure);
        const uint32_t ncuts = mj_cutoffs(measure, cuts);
        for (uint32_t c = 0; c < ncuts; ++c) {
            uint64_t w[MATCH_JOIN_LENGTHS];
            mj_need_mask(measure, cuts[c], w);
            for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq)
                for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc)
                    masks += (((w[lq] >> lc) & 1ull) != 0ull) != (match_join_ub(measure, lq, lc) >= cuts[c]);
        }
    }
    const uint32_t failed = mj_replay_all();
    printf("match_join harness: %u length pairs off their bound, %u mask bits differ, %u replays failed\n", bounds, masks, failed);
    return bounds || masks || failed ? 1 : 0;
}
#endif
