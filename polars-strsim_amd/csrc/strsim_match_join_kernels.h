// strsim_match_join_kernels.h -- the sweep of strsim_match_join_device (the rule is in strsim_match_join.h).
// Included by strsim_kernels.hip inside namespace strsim, after strsim_join_kernels.h: everything around the sweep -- the pack, the
// length order, k_join_totals, the 64-bit scan, k_join_slow and k_join_sort_rows -- is the threshold join's own, and so is the body
// of the sweep itself (join_lane_start / join_lane_slice / join_lane_end of strsim_join_kernels.h: the lane's query, the slice of a
// length bucket, the hit map, the count or the store into the lane's segment).
//
//   k_match_join_lane<M, FILL>   adds the quotient table in LDS for measures 0 .. 2, the visiting order and k_match_lane's scoring.
//                       A lane reads its word of the need mask once, the wave ORs the words of its live lanes and visits exactly the
//                       lengths whose bit is set, in ascending order.  A pair yields its f64 score (match_score), which is also
//                       what is stored (MatchJoinRule).
//
// No atomics, every loop is bounded by the kernel's arguments, no workgroup waits on another, every store is a plain vector store.
#pragma once

// MatchJoinRule with k_match_lane's scoring call: the f64 score of the pair (s_q: the quotient table in LDS).
template <int MEASURE>
struct MatchJoinSweep : MatchJoinRule {
    const double *s_q;
    template <int NP>
    __device__ __forceinline__ double core(const uint32_t (&wt)[8], uint32_t lc, const uint32_t (&P)[NP], uint32_t w0, uint32_t lq, uint32_t) const
    {
        return match_score<MEASURE, NP>(s_q, wt, lc, P, w0, lq);
    }
};

// Grid: (ceil(nq / MATCH_BLOCK), splits).  The arguments of k_join_lane with the quotient table, the need mask and min_score where
// the rank table and rlimit stood.
template <int MEASURE, bool FILL>
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_join_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                                 const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qstart,
                                                                 uint32_t nq, const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                                 const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ cstart,
                                                                 const double *__restrict__ qtab, const MatchJoinNeed need_mask, double min_score,
                                                                 uint32_t upper_flag, uint32_t *__restrict__ cnt, uint32_t *__restrict__ map,
                                                                 uint64_t map_words, uint32_t map_shift, const uint64_t *__restrict__ indptr,
                                                                 uint32_t *__restrict__ out_index, double *__restrict__ out_score)
{
    constexpr bool TABLE = MEASURE == LEVENSHTEIN || MEASURE == JARO || MEASURE == JARO_WINKLER;
    __shared__ double s_q[TABLE ? QTAB_N * QTAB_N : 1];
    if (TABLE)
        for (uint32_t x = threadIdx.x; x < (uint32_t)(QTAB_N * QTAB_N); x += MATCH_BLOCK) s_q[x] = qtab[x];
    __syncthreads();

    const JoinSweep s{qwords, qmeta, qperm, qstart, nq, sw, sm, sidx, cstart, upper_flag != 0u, cnt, map, map_words, map_shift, indptr,
                      out_index, out_score};
    JoinLane L;
    join_lane_start<FILL>(s, L);

    // the lane's word of the need mask and the wave's: every index into the mask is uniform (the argument stays in scalar registers)
    uint64_t mine = 0ull, wave = 0ull;
    for (uint32_t l = 0; l < MATCH_JOIN_LENGTHS; ++l) {
        const uint64_t w = need_mask.w[l];
        const bool is = L.live && L.lq == l;
        if (is) mine = w;
        if (__ballot(is) != 0ull) wave |= w;
    }

    const MatchJoinSweep<MEASURE> R{{min_score}, s_q};
    for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
        if (!((wave >> lc) & 1ull)) continue; // (uniform) no live lane can have a hit at this length
        const bool need = ((mine >> lc) & 1ull) != 0ull;
        join_lane_slice<FILL>(s, L, lc, need, R);
    }
    join_lane_end<FILL>(s, L);
}
