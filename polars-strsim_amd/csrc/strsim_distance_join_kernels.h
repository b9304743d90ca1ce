// strsim_distance_join_kernels.h -- the sweep of strsim_distance_join_device (the rules are in strsim_distance_join.h; DESIGN.md
// section 27).  Included by strsim_kernels.hip inside namespace strsim, after strsim_match_join_kernels.h: everything around the
// sweep is the threshold join's own, and so is the body of the sweep itself (join_lane_start / join_lane_slice / join_lane_end of
// strsim_join_kernels.h).
//
//   k_distance_join_lane<KIND, FILL>  k_match_join_lane's skeleton -- the lane's word of the need mask, the wave's, the lengths
//                       whose bit is set in ascending order -- with an integer edit distance as its scoring call: the lane's query
//                       is the pattern, the candidate the wave-uniform text.  Levenshtein and OSA: nearest_lev_uniform_text /
//                       nearest_osa_uniform_text as they are, no LDS.  Damerau-Levenshtein: the OSA distance of every visited
//                       candidate, and when some lane of the wave is left undecided by it (distance_join_undecided) one run of
//                       dl_lane_core for the wave, the other lanes' cells predicated off.  The lane's column records are one
//                       dword a column in LDS, laid out [column][lane] as in k_dl_lane: 32 KB a workgroup.
//   k_distance_join_finish            the hits' f64 values -(double)d into the uint32 distances of the caller's column.
//
// No atomics, every loop is bounded by the kernel's arguments, no workgroup waits on another, every store is a plain vector store.
#pragma once

// DistanceJoinRule with the bit-parallel scoring call (TR: OSA instead of Levenshtein): the distance of the pair.
template <bool TR>
struct DistanceJoinSweep : DistanceJoinRule {
    template <int NP>
    __device__ __forceinline__ uint32_t core(const uint32_t (&wt)[8], uint32_t lc, const uint32_t (&P)[NP], uint32_t, uint32_t lq, uint32_t) const
    {
        return TR ? nearest_osa_uniform_text<NP>(wt, lc, P, lq) : nearest_lev_uniform_text<NP>(wt, lc, P, lq);
    }
};

// What the Damerau-Levenshtein scoring call hands on: the OSA distance and the candidate it belongs to.  Both plane forms return
// the same uniform text, so it stays in scalar registers behind the slice's branch between them.
struct DamerauJoinOsa {
    uint32_t o, lc;
    uint32_t wt[8];
};

// The rule of the Damerau-Levenshtein sweep.  core() is the OSA column; value() runs where the wave has converged again: the filter
// per lane, and the cell DP once for the wave when any lane is undecided.  wq: the lane's own query words, live / lq: the lane's,
// pmax: the longest live query of the wave (uniform, the DP's row bound), col: the lane's column records in LDS.
struct DamerauJoinSweep {
    uint32_t kmax;
    bool live;
    uint32_t lq, pmax;
    uint32_t wq[8];
    uint32_t *col;
    template <int NP>
    __device__ __forceinline__ DamerauJoinOsa core(const uint32_t (&wt)[8], uint32_t lc, const uint32_t (&P)[NP], uint32_t, uint32_t lq_, uint32_t) const
    {
        return DamerauJoinOsa{nearest_osa_uniform_text<NP>(wt, lc, P, lq_), lc, {wt[0], wt[1], wt[2], wt[3], wt[4], wt[5], wt[6], wt[7]}};
    }
    __device__ __forceinline__ uint32_t value(const DamerauJoinOsa &c) const
    {
        const bool und = live && distance_join_needs(lq, c.lc, kmax) && distance_join_undecided(c.o, kmax);
        if (__ballot(und) == 0ull) return c.o; // (uniform)
        STRSIM_CHECK_RANGE(K_DAMERAU, 30, lq, pmax, 0, DL_LANE_MAX);
        STRSIM_CHECK_RANGE(K_DAMERAU, 31, lq, c.lc, 0, DL_LANE_MAX);
        STRSIM_CHECK_INDEX(K_DAMERAU, 32, lq, (c.lc ? c.lc - 1u : 0u) * MATCH_BLOCK + threadIdx.x, DL_LANE_MAX * MATCH_BLOCK);
        const uint32_t d = dl_lane_core(wq, und ? lq : 0u, pmax, c.wt, c.lc, c.lc, col, MATCH_BLOCK);
        return und ? d : c.o;
    }
    __device__ __forceinline__ bool hit(uint32_t d, bool upper, uint32_t i, uint32_t j) const { return distance_join_hit(d, kmax, upper, i, j); }
    __device__ __forceinline__ double score(uint32_t d) const { return -(double)d; }
};

// The lengths of the wave's need words in ascending order under the rule R, and the lane's count.
template <bool FILL, class Rule>
__device__ __forceinline__ void distance_join_lengths(const JoinSweep &s, JoinLane &L, const MatchJoinNeed &need_mask, const Rule &R)
{
    // the lane's word of the need mask and the wave's: every index into the mask is uniform (the argument stays in scalar registers)
    uint64_t mine = 0ull, wave = 0ull;
    for (uint32_t l = 0; l < MATCH_JOIN_LENGTHS; ++l) {
        const uint64_t w = need_mask.w[l];
        const bool is = L.live && L.lq == l;
        if (is) mine = w;
        if (__ballot(is) != 0ull) wave |= w;
    }
    for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
        if (!((wave >> lc) & 1ull)) continue; // (uniform) no live lane can have a hit at this length
        const bool need = ((mine >> lc) & 1ull) != 0ull;
        join_lane_slice<FILL>(s, L, lc, need, R);
    }
    join_lane_end<FILL>(s, L);
}

// Grid: (ceil(nq / MATCH_BLOCK), splits).  The arguments of k_match_join_lane with the integer cutoff where the quotient table and
// min_score stood.  KIND: EDIT_LEVENSHTEIN, EDIT_OSA or EDIT_DAMERAU.
template <int KIND, bool FILL>
__global__ __launch_bounds__(MATCH_BLOCK) void k_distance_join_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                                    const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qstart,
                                                                    uint32_t nq, const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                                    const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ cstart,
                                                                    const MatchJoinNeed need_mask, uint32_t kmax, uint32_t upper_flag,
                                                                    uint32_t *__restrict__ cnt, uint32_t *__restrict__ map, uint64_t map_words,
                                                                    uint32_t map_shift, const uint64_t *__restrict__ indptr,
                                                                    uint32_t *__restrict__ out_index, double *__restrict__ out_score)
{
    const JoinSweep s{qwords, qmeta, qperm, qstart, nq, sw, sm, sidx, cstart, upper_flag != 0u, cnt, map, map_words, map_shift, indptr,
                      out_index, out_score};
    JoinLane L;
    join_lane_start<FILL>(s, L);
    if constexpr (KIND == EDIT_DAMERAU) {
        __shared__ uint32_t s_col[DL_LANE_MAX * MATCH_BLOCK]; // [column][lane]: a wave reads and writes 64 consecutive dwords
        DamerauJoinSweep R{kmax, L.live, L.lq, nearest_wave_max(L.live ? L.lq : 0u), {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, s_col + threadIdx.x};
        if (L.live) { // the lane's own query words again (the lane's planes do not give a byte back)
            const uint4 *const src = reinterpret_cast<const uint4 *>(qwords + (size_t)L.i * 8u);
            const uint4 a = src[0], b = src[1];
            R.wq[0] = a.x; R.wq[1] = a.y; R.wq[2] = a.z; R.wq[3] = a.w; R.wq[4] = b.x; R.wq[5] = b.y; R.wq[6] = b.z; R.wq[7] = b.w;
        }
        distance_join_lengths<FILL>(s, L, need_mask, R);
    } else {
        const DistanceJoinSweep<KIND == EDIT_OSA> R{{kmax}};
        distance_join_lengths<FILL>(s, L, need_mask, R);
    }
}

__global__ __launch_bounds__(MATCH_BLOCK) void k_distance_join_finish(const double *__restrict__ score, uint64_t n, uint32_t *__restrict__ dist)
{
    const uint64_t x = (uint64_t)blockIdx.x * MATCH_BLOCK + threadIdx.x;
    if (x < n) dist[x] = (uint32_t)(-score[x]);
}
