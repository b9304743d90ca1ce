// strsim_match_join.h -- threshold join by the five reference measures: every pair (query i, candidate j) with
// score(i, j) >= min_score, as CSR in ascending candidate index (strsim_match_join_device).  score = one of
// normalised Levenshtein, Jaro, Jaro-Winkler, multiset Jaccard and Sorensen-Dice, bit for bit the pairwise call's.
//
// The protocol is strsim_join.h's, unchanged: the length order, two sweeps (count, fill) with the hit map between them, the
// per-(split, query) counts and their prefix, the 64-bit scan, the fallback for strings outside the lane class and the row sort.
// The sweep's body is the join's too (join_lane_start / _slice / _end of strsim_join_kernels.h).  This header holds what differs
// and what the host shares with the kernel (tests/cpu_harness/match_join_harness.cpp compiles it with g++): the pruning rule, and
// the rule object that tells that body what a pair yields here (MatchJoinRule).
//
// Pruning (exact).  The scores are f64 values without a rank table, so the bound of a length pair is the measure's OWN epilogue at
// the best integers the lengths allow -- the same function the kernels end in, never a separately rounded expression:
//   Levenshtein    d >= |lq - lc|                          -> epilogue_levenshtein(|lq - lc|, lq, lc)
//   Jaro           m <= mn = min(lq, lc), t >= 0           -> epilogue_jaro(mn, 0, lq, lc)
//   Jaro-Winkler   the same, prefix <= min(4, mn)          -> epilogue_jaro_winkler(epilogue_jaro(mn, 0, lq, lc), min(4, mn))
//   Jaccard / Sorensen-Dice   isect <= mn                  -> epilogue_jaccard / epilogue_sorensen_dice(mn, lq, lc)
// and 1.0 for two empty strings, 0.0 for exactly one.  Every epilogue is monotone in each of its integers over the range the kernel
// can produce (the harness checks the maximum over EVERY tuple for all lengths 0 .. 32), so no pair of these lengths scores above
// match_join_ub and some tuple attains it.  A lane needs length lc iff match_join_ub(measure, lq, lc) >= min_score: the comparison
// the kernel makes with a score, made with the bound.  The host builds the 33 words of that relation per call (MatchJoinNeed, 1 089
// compares) and passes them as a kernel argument: no device work, no wait, no scratch.  There is no shrinking top-k bound here, so
// the kernel needs no window and no nearest-first stepping: a wave ORs the words of its live lanes and visits exactly the lengths
// whose bit is set, in ascending order.
#pragma once
#include <stdint.h>

#include "strsim_join.h"

namespace strsim {

constexpr uint32_t MATCH_JOIN_LENGTHS = 33u; // lengths 0 .. 32 of the lane class

// The best score a pair of lengths (lq, lc), both <= 32, can have by `measure` (0 .. 4).
STRSIM_HD double match_join_ub(int measure, uint32_t lq, uint32_t lc)
{
    if (lq == 0u && lc == 0u) return 1.0;
    if (lq == 0u || lc == 0u) return 0.0;
    const uint32_t mn = lq < lc ? lq : lc;
    switch (measure) {
    case LEVENSHTEIN: return epilogue_levenshtein(lq > lc ? lq - lc : lc - lq, lq, lc);
    case JARO: return epilogue_jaro(mn, 0u, lq, lc);
    case JARO_WINKLER: return epilogue_jaro_winkler(epilogue_jaro(mn, 0u, lq, lc), mn < 4u ? mn : 4u);
    case JACCARD: return epilogue_jaccard(mn, lq, lc);
    default: return epilogue_sorensen_dice(mn, lq, lc);
    }
}

// need.w[lq]: bit lc is set iff a query of length lq can have a hit among the candidates of length lc.
struct MatchJoinNeed {
    uint64_t w[MATCH_JOIN_LENGTHS];
};

STRSIM_HD bool match_join_needs(const MatchJoinNeed &need, uint32_t lq, uint32_t lc) { return ((need.w[lq] >> lc) & 1ull) != 0ull; }

// The need mask of a call; returns whether any pair of lengths can hit at all (false: the cutoff is above every score).
inline bool match_join_need_mask(int measure, double min_score, MatchJoinNeed &need)
{
    uint64_t any = 0ull;
    for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq) {
        uint64_t w = 0ull;
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc)
            if (match_join_ub(measure, lq, lc) >= min_score) w |= 1ull << lc;
        need.w[lq] = w;
        any |= w;
    }
    return any != 0ull;
}

// Whether pair (i, j) of score v is reported.
STRSIM_HD bool match_join_hit(double v, double min_score, bool upper, uint32_t i, uint32_t j) { return v >= min_score && (!upper || j > i); }

// The rule object of the shared sweep (join_lane_slice, where JoinRankRule stands for the rank join): a pair yields its f64 score,
// which is what is stored.
struct MatchJoinRule {
    double min_score;
    STRSIM_HD double value(double v) const { return v; }
    STRSIM_HD bool hit(double v, bool upper, uint32_t i, uint32_t j) const { return match_join_hit(v, min_score, upper, i, j); }
    STRSIM_HD double score(double v) const { return v; }
};

} // namespace strsim
