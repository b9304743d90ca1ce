// strsim_qgram_join_kernels.h -- the sweep of strsim_qgram_join_device (the rule and the scoring call are in strsim_qgram_join.h;
// DESIGN.md section 25).  Included by strsim_kernels.hip inside namespace strsim, after strsim_match_join_kernels.h: everything
// around the sweep is the threshold join's own, and so is the body of the sweep itself (join_lane_start / join_lane_slice /
// join_lane_end of strsim_join_kernels.h).
//
//   k_qgram_join_first<Q>           set mode only, once per call behind the length order: one thread per fast candidate in that
//                       order, the first occurrences among its grams into one word (qgram_join_first over its own planes).
//   k_qgram_join_lane<Q, SET, FILL>  k_match_join_lane's skeleton -- the lane's word of the need mask, the wave's, the lengths whose
//                       bit is set in ascending order -- with the q-gram scoring call: the lane's query is the pattern, the
//                       candidate the wave-uniform text (qgram_join_pair).  Set mode: the number of distinct grams of the lane's
//                       query once before the length loop, the candidate's word of first occurrences through a scalar load at the
//                       position the slice hands the rule.  `kind` is used once, in the epilogue.
//
// No atomics, every loop is bounded by the kernel's arguments, no workgroup waits on another, every store is a plain vector store.
#pragma once

// Grid: ceil(nc / MATCH_BLOCK).  The fast candidates are the first cstart[NEAREST_SLOW_BUCKET] positions of the length order.
template <int Q>
__global__ __launch_bounds__(MATCH_BLOCK) void k_qgram_join_first(const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                                  const uint32_t *__restrict__ cstart, uint32_t nc,
                                                                  uint32_t *__restrict__ first)
{
    const uint32_t x = blockIdx.x * MATCH_BLOCK + threadIdx.x;
    const uint32_t fast = cstart[NEAREST_SLOW_BUCKET];
    const bool live = x < nc && x < fast;
    const uint32_t len = live ? sm[x] & 63u : 0u;
    uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (live) {
        const uint4 *const src = reinterpret_cast<const uint4 *>(sw + (size_t)x * 8u);
        const uint4 a = src[0], b = src[1];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    }
    uint32_t P[7];
    build_planes<7>(w, P);
    const uint32_t f = qgram_join_first<Q>(w, P, len, nearest_wave_max(len));
    if (live) first[x] = f;
}

// MatchJoinRule with the q-gram scoring call: the f64 score of the pair.  first: the candidates' words of first occurrences in
// length order (set mode), nbq: the distinct grams of the lane's query (set mode).
template <int Q, bool SET>
struct QgramJoinSweep : MatchJoinRule {
    int kind;
    const uint32_t *first;
    uint32_t nbq;
    template <int NP>
    __device__ __forceinline__ double core(const uint32_t (&wt)[8], uint32_t lc, const uint32_t (&P)[NP], uint32_t w0, uint32_t lq,
                                           uint32_t x) const
    {
        const uint32_t first_c = SET ? first[x] : 0u; // (x is uniform: a scalar load)
        return qgram_join_pair<NP, Q, SET>(kind, wt, lc, first_c, P, w0, lq, nbq);
    }
};

// Grid: (ceil(nq / MATCH_BLOCK), splits).  The arguments of k_match_join_lane with the kind and the first occurrences where the
// quotient table stood.
template <int Q, bool SET, bool FILL>
__global__ __launch_bounds__(MATCH_BLOCK) void k_qgram_join_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                                 const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qstart,
                                                                 uint32_t nq, const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                                 const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ cstart,
                                                                 int kind, const uint32_t *__restrict__ first, const MatchJoinNeed need_mask,
                                                                 double min_score, uint32_t upper_flag, uint32_t *__restrict__ cnt,
                                                                 uint32_t *__restrict__ map, uint64_t map_words, uint32_t map_shift,
                                                                 const uint64_t *__restrict__ indptr, uint32_t *__restrict__ out_index,
                                                                 double *__restrict__ out_score)
{
    const JoinSweep s{qwords, qmeta, qperm, qstart, nq, sw, sm, sidx, cstart, upper_flag != 0u, cnt, map, map_words, map_shift, indptr,
                      out_index, out_score};
    JoinLane L;
    join_lane_start<FILL>(s, L);

    // set mode: the distinct grams of the lane's query, from its eight words again and its own planes
    uint32_t nbq = 0u;
    if constexpr (SET) {
        uint32_t wq[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (L.live) {
            const uint4 *const src = reinterpret_cast<const uint4 *>(qwords + (size_t)L.i * 8u);
            const uint4 a = src[0], b = src[1];
            wq[0] = a.x; wq[1] = a.y; wq[2] = a.z; wq[3] = a.w; wq[4] = b.x; wq[5] = b.y; wq[6] = b.z; wq[7] = b.w;
        }
        nbq = popc32(qgram_join_first<Q>(wq, L.q.P, L.lq, nearest_wave_max(L.lq)));
    }

    // the lane's word of the need mask and the wave's: every index into the mask is uniform (the argument stays in scalar registers)
    uint64_t mine = 0ull, wave = 0ull;
    for (uint32_t l = 0; l < MATCH_JOIN_LENGTHS; ++l) {
        const uint64_t w = need_mask.w[l];
        const bool is = L.live && L.lq == l;
        if (is) mine = w;
        if (__ballot(is) != 0ull) wave |= w;
    }

    const QgramJoinSweep<Q, SET> R{{min_score}, kind, first, nbq};
    for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
        if (!((wave >> lc) & 1ull)) continue; // (uniform) no live lane can have a hit at this length
        const bool need = ((mine >> lc) & 1ull) != 0ull;
        join_lane_slice<FILL>(s, L, lc, need, R);
    }
    join_lane_end<FILL>(s, L);
}
