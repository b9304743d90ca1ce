// strsim_qgram_join.h -- threshold join by q-gram similarity: every pair (query i, candidate j) with
// qgram_score(kind, q, mode)(i, j) >= min_score, as CSR in ascending candidate index (strsim_qgram_join_device, DESIGN.md section
// 25).  The score is bit for bit strsim_qgram_device's for that pair.
//
// The protocol is strsim_join.h's and the sweep's body is the join's (join_lane_start / _slice / _end of strsim_join_kernels.h), as
// for strsim_match_join.h, whose need mask (MatchJoinNeed, match_join_needs) and rule object (MatchJoinRule) are used as they are.
// This header holds what differs and what the host shares with the kernel (tests/cpu_harness/qgram_join_harness.cpp compiles it
// with g++): the pruning rule and the scoring call of one lane-class pair.
//
// Pruning (exact).  The bound of a length pair is the library's own qgram_score at the best integers the lengths allow, never a
// separately rounded expression.  With gq = qgram_count(lq, q), gc = qgram_count(lc, q):
//   both 0          1.0 when lq == lc (the strings can be equal), else 0.0
//   exactly one 0   0.0
//   multiset mode   I <= min(gq, gc), na = gq, nb = gc   -> qgram_score(kind, min(gq, gc), gq, gc, false).  Every kind grows with I
//                   at fixed counts.  Jaccard, Sorensen-Dice and cosine fall below 1.0 as soon as the counts differ; OVERLAP
//                   divides by min(na, nb), so its bound is 1.0 at every pair of lengths with a gram each: overlap is never pruned.
//   set mode        the counts are those of the DISTINCT grams, which the lengths do not fix ("aaaa" and "aa" at q = 2 have one
//                   gram each and score 1.0 by every kind): the bound is qgram_score(kind, 1, 1, 1, false) = 1.0 whenever both
//                   strings have a gram.  Set mode is not pruned by length.
// A lane needs length lc iff qgram_join_ub(kind, q, set, lq, lc) >= min_score; the host builds the 33 words of that relation per
// call and passes them as a kernel argument, as match_join_need_mask does.
//
// The scoring call.  The QUERY is the pattern: its planes are the lane's (LaneQuery), one 32-bit word each.  The CANDIDATE is the
// text, wave-uniform: E(c_j) is eq_mask of a scalar byte, and the gram masks are qgram_walk's recurrence (QgramGrams of
// strsim_qgram.h: the one step both share) cut to the query's gq grams.  The loop ends at lc, so no byte behind the text is looked
// at and padding forms no gram; a NUL inside a string is a character.  The scores are symmetric in their two strings, so the roles
// are free.  Multiset: I is the greedy of qgram_walk<QGRAM_GREEDY> (qgram_take), na = gc, nb = gq.  Set: the candidate's first
// occurrences first_c (one word per candidate, computed once per call by k_qgram_join_first and read through a scalar load) give
// na = popc(first_c) and I = the first occurrences whose gram mask is not empty; nb, the query's distinct grams, depends on the lane
// alone and is computed once per lane (qgram_join_first over the query's own planes).
#pragma once
#include <stdint.h>

#include "strsim_match_join.h"
#include "strsim_qgram.h"

namespace strsim {

// The best score a pair of byte lengths (lq, lc), both <= 32 and ASCII, can have by `kind` over q-grams in the given mode.
STRSIM_HD double qgram_join_ub(int kind, uint32_t q, bool set, uint32_t lq, uint32_t lc)
{
    const uint32_t gq = qgram_count(lq, q), gc = qgram_count(lc, q);
    if (gq == 0u && gc == 0u) return lq == lc ? 1.0 : 0.0;
    if (gq == 0u || gc == 0u) return 0.0;
    if (set) return qgram_score(kind, 1u, 1u, 1u, false);
    return qgram_score(kind, gq < gc ? gq : gc, gq, gc, false);
}

// The need mask of a call; returns whether any pair of lengths can hit at all (false: the cutoff is above every score).
inline bool qgram_join_need_mask(int kind, uint32_t q, bool set, double min_score, MatchJoinNeed &need)
{
    uint64_t any = 0ull;
    for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq) {
        uint64_t w = 0ull;
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc)
            if (qgram_join_ub(kind, q, set, lq, lc) >= min_score) w |= 1ull << lc;
        need.w[lq] = w;
        any |= w;
    }
    return any != 0ull;
}

// The first occurrences among the grams of a string of len <= 32 ASCII bytes: w its eight words (zeros behind it), P the seven
// planes of those words, tmax >= len the same in every lane.  Bit i: gram i equals no gram below it.
template <int Q>
STRSIM_HD uint32_t qgram_join_first(const uint32_t (&w)[8], const uint32_t (&P)[7], uint32_t len, uint32_t tmax)
{
    const uint32_t wt[16] = {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const uint32_t none[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const uint32_t seen = (uint32_t)qgram_walk<uint32_t, Q, QGRAM_SEEN>(wt, len, tmax, P, none, 0u);
    return ~seen & low_ones(qgram_count(len, (uint32_t)Q));
}

// I of one pair: the text wt (lc bytes, the same in every lane) against the NP planes P of the pattern, whose first gq grams
// count.  Multiset: the greedy count.  Set: the text's first occurrences (first_c) that equal a pattern gram.
template <int NP, int Q, bool SET>
STRSIM_HD uint32_t qgram_join_isect(const uint32_t (&wt)[8], uint32_t lc, const uint32_t (&P)[NP], uint32_t gq, uint32_t first_c)
{
    const uint32_t rows = low_ones(gq);
    QgramGrams<uint32_t, Q> grams;
    uint32_t used = 0u, res = 0u;
    for (uint32_t w = 0; w < (lc + 3u) / 4u; ++w) unrolled_until<0, 4>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        const uint32_t j = 4u * w + (uint32_t)b;
        if (j >= lc) return false;
        const uint32_t E = eq_mask<NP>(P, 0xFFFFFFFFu, wt[w], b);
        const uint32_t M = grams.gram(E) & rows;
        if constexpr (SET) {
            // (the gram that byte j completes starts at j - Q + 1; before the first one M is empty and the bit read is not used)
            const uint32_t first = (first_c >> ((j + 32u - (uint32_t)(Q - 1)) & 31u)) & 1u;
            res += M != 0u ? first : 0u;
        } else {
            (void)first_c;
            res += qgram_take<uint32_t>(M, used);
        }
        grams.push(E);
        return true;
    });
    return res;
}

// The f64 score of one pair as the sweep computes it.  Query: planes P, first word w0, lq bytes, nbq distinct grams (set mode
// only).  Candidate: text wt, lc bytes, first occurrences first_c (set mode only).
template <int NP, int Q, bool SET>
STRSIM_HD double qgram_join_pair(int kind, const uint32_t (&wt)[8], uint32_t lc, uint32_t first_c, const uint32_t (&P)[NP], uint32_t w0,
                                 uint32_t lq, uint32_t nbq)
{
    const uint32_t gq = qgram_count(lq, (uint32_t)Q), gc = qgram_count(lc, (uint32_t)Q);
    const uint32_t isect = qgram_join_isect<NP, Q, SET>(wt, lc, P, gq, first_c);
    // equal and both shorter than q (at most two bytes: both fit the first word, the rest of it is zero)
    const bool same = lq == lc && lc < (uint32_t)Q && w0 == wt[0];
    return qgram_score(kind, isect, SET ? popc32(first_c) : gc, SET ? nbq : gq, same);
}

} // namespace strsim
