// strsim_distance_join.h -- join by integer edit distance: every pair (query i, candidate j) with d(i, j) <= k, as CSR in ascending
// candidate index (strsim_distance_join_device).  d is the Levenshtein, the OSA or the unrestricted
// Damerau-Levenshtein distance over Unicode scalar values: exactly what strsim_distance_device and strsim_damerau_distance_device
// return without a cutoff.
//
// The protocol is strsim_join.h's and the sweep's body is the join's (join_lane_start / _slice / _end of strsim_join_kernels.h), as
// for strsim_match_join.h, whose need mask (MatchJoinNeed) is used as it is.  This header holds what differs and what the host
// shares with the kernel (tests/cpu_harness/distance_join_harness.cpp compiles it with g++): the pruning rule, the rule object and
// the filter of the Damerau-Levenshtein sweep.
//
// Inside the join a hit carries the f64 value -(double)d, as the nearest search's lists do: v >= -(double)k is d <= k, -INFINITY
// is no cutoff, and the fallback, the row sort and cluster_labels work on it unchanged.  Every d and every k is below 2^32, so the
// conversion is exact both ways.
//
// Pruning (exact).  An edit changes the length by at most one and a swap not at all, so d >= |lq - lc| by all three measures: a
// pair whose lengths differ by more than k is no hit, and a lane needs length lc iff |lq - lc| <= k.  The host builds the 33 words
// of that relation per call (distance_join_need_mask); the wave visits the union of its live lanes' words.
//
// Damerau-Levenshtein (exact by filter and verify).  With o the OSA distance of the pair and dl the unrestricted one:
//   (1) dl <= o                every OSA script is a Damerau-Levenshtein script
//   (2) o <= 2 -> dl == o      dl = 0 iff the strings are equal iff o = 0; a script of one edit is an OSA script, so dl = 1 iff o = 1;
//                              so o = 2 leaves dl = 2
//   (3) o <= 2 dl              o <= lev, and Levenshtein replaces a swap across a gap (cost 1 + |x| + |y|) by two substitutions
//                              and the same |x| + |y| edits (2 + |x| + |y|), at most twice the cost: lev <= 2 dl
// so per candidate: o <= 2 is decided (d = o); o > 2 k is decided (dl >= ceil(o / 2) > k: no hit); 3 <= o <= 2 k is undecided and
// the cell DP of strsim_damerau.h (dl_lane_core) runs.  At k <= 1 nothing is ever undecided.
#pragma once
#include <stdint.h>

#include "strsim_damerau.h"
#include "strsim_match_join.h"
#include "strsim_nearest.h"

namespace strsim {

enum EditKind : int { EDIT_LEVENSHTEIN = 0, EDIT_OSA = 1, EDIT_DAMERAU = 2 }; // = STRSIM_EDIT_*

// The cutoff of the join's f64 plumbing for the integer cutoff k.
inline double distance_join_cutoff(uint32_t k) { return k == DIST_UNBOUNDED ? -__builtin_inf() : -(double)k; }

// Whether a query of length lq can have a hit among the candidates of length lc: d >= |lq - lc|.
STRSIM_HD bool distance_join_needs(uint32_t lq, uint32_t lc, uint32_t k) { return nearest_needs(lq, lc, k); }

// The need mask of a call (every (lq, lq) is set: there is no k above which nothing can hit).
inline void distance_join_need_mask(uint32_t k, MatchJoinNeed &need)
{
    for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq) {
        uint64_t w = 0ull;
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc)
            if (distance_join_needs(lq, lc, k)) w |= 1ull << lc;
        need.w[lq] = w;
    }
}

// Whether pair (i, j) at distance d is reported.
STRSIM_HD bool distance_join_hit(uint32_t d, uint32_t k, bool upper, uint32_t i, uint32_t j) { return d <= k && (!upper || j > i); }

// The rule object of the shared sweep (join_lane_slice): a pair yields its distance, -(double)d is what is stored.
struct DistanceJoinRule {
    uint32_t kmax;
    STRSIM_HD uint32_t value(uint32_t d) const { return d; }
    STRSIM_HD bool hit(uint32_t d, bool upper, uint32_t i, uint32_t j) const { return distance_join_hit(d, kmax, upper, i, j); }
    STRSIM_HD double score(uint32_t d) const { return -(double)d; }
};

// The filter of the Damerau-Levenshtein sweep: whether the OSA distance o leaves dl <= k open (3 <= o <= 2 k, without overflow at
// k = DIST_UNBOUNDED).  Otherwise d = o stands: it is dl when o <= 2, and a bound above k that is no hit when o > 2 k.
STRSIM_HD bool distance_join_undecided(uint32_t o, uint32_t k) { return o > 2u && (o + 1u) / 2u <= k; }

// d of one lane-class pair as the Damerau-Levenshtein sweep forms it: the OSA distance o where the filter decides, the cell DP's
// value otherwise.  wq / lq: the query (the rows), wt / lc: the candidate (the columns); col and stride as in dl_lane_core.
STRSIM_HD uint32_t distance_join_damerau_pair(uint32_t o, uint32_t k, const uint32_t (&wq)[8], uint32_t lq, const uint32_t (&wt)[8], uint32_t lc,
                                              uint32_t *col, uint32_t stride)
{
    if (!distance_join_needs(lq, lc, k) || !distance_join_undecided(o, k)) return o;
    return dl_lane_core(wq, lq, lq, wt, lc, lc, col, stride);
}

} // namespace strsim
