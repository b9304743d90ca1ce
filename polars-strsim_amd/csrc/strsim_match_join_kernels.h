// strsim_match_join_kernels.h -- the sweep of strsim_match_join_device (the rule is in strsim_match_join.h).
// Included by strsim_kernels.hip inside namespace strsim, after strsim_join_kernels.h: everything around the sweep -- the pack, the
// length order, k_join_totals, the 64-bit scan, k_join_slow and k_join_sort_rows -- is the threshold join's own.
//
//   k_match_join_lane<M, FILL>   k_join_lane's skeleton with k_match_lane's scoring.  ONE QUERY PER LANE in length order, its
//                       bit-planes in registers (match_lane_query), the candidate wave-uniform text through scalar loads, the
//                       quotient table in LDS for measures 0 .. 2.  blockIdx.y takes its slice of every length bucket.  A lane reads
//                       its word of the need mask once, the wave ORs the words of its live lanes and visits exactly the lengths
//                       whose bit is set, in ascending order.  FILL = false counts a lane's hits in a register, stores one count per
//                       (split, query) and marks the wave's hit map; FILL = true computes the marked candidates only and stores
//                       (j, score) into the lane's own segment, the cursor compared with the segment's end before every store.
//
// No atomics, every loop is bounded by the kernel's arguments, no workgroup waits on another, every store is a plain vector store.
#pragma once

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

    // the last positions of the length order first: the longest queries meet the longest candidates
    const uint32_t p = (gridDim.x - 1u - blockIdx.x) * MATCH_BLOCK + threadIdx.x;
    const uint32_t split = blockIdx.y, splits = gridDim.y;
    const bool upper = upper_flag != 0u;
    const bool have = p < nq;
    const uint32_t i = have ? qperm[p] : 0u;
    const bool live = have && p < qstart[NEAREST_SLOW_BUCKET];
    const uint32_t qm = live ? qmeta[i] : 0u;
    const uint32_t lq = qm & 63u;
    const LaneQuery q = match_lane_query(qwords, i, live, qm);

    // the lane's word of the need mask and the wave's: every index into the mask is uniform (the argument stays in scalar registers)
    uint64_t mine = 0ull, wave = 0ull;
    for (uint32_t l = 0; l < MATCH_JOIN_LENGTHS; ++l) {
        const uint64_t w = need_mask.w[l];
        const bool is = live && lq == l;
        if (is) mine = w;
        if (__ballot(is) != 0ull) wave |= w;
    }

    uint32_t *const wmap = map + (size_t)(p >> 6) * map_words; // the wave's hit map (strsim_join.h)
    const bool lane0 = (threadIdx.x & 63u) == 0u;
    uint32_t count = 0u;
    uint64_t cur = 0u, end = 0u; // FILL: the lane's segment (empty unless live)
    if (FILL && live) {
        const uint64_t base = indptr[i];
        cur = base + cnt[(size_t)split * nq + i];
        end = base + cnt[(size_t)(split + 1u) * nq + i]; // (list `splits` is the fallback's: the row always exists)
    }

    for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
        if (!((wave >> lc) & 1ull)) continue; // (uniform) no live lane can have a hit at this length
        const bool need = ((mine >> lc) & 1ull) != 0ull; // of (lq, lc) alone: out of the candidate loop
        const uint32_t c0 = cstart[lc], n = cstart[lc + 1u] - c0;
        uint32_t x0, x1;
        join_slice(c0, n, split, splits, x0, x1);
        const uint32_t k = join_map_slice(lc, split, splits);
        uint64_t at = ~0ull; // the word of the hit map in hand (uniform), its bits
        uint32_t bits = 0u;
        for (uint32_t x = x0; x < x1; ++x) { // (uniform: scalar loads)
            const uint64_t w = join_map_word(x, map_shift, k);
            if (w != at) {
                if (!FILL && at != ~0ull && lane0) wmap[at] = bits;
                at = w;
                bits = FILL ? wave_uniform(wmap[w]) : 0u;
            }
            const uint32_t bit = join_map_bit(x, map_shift);
            if (FILL && !(bits & bit)) continue; // no lane of the wave had a hit in this group
            const uint32_t cm = sm[x], j = sidx[x];
            uint32_t wt[8];
#pragma unroll
            for (int w = 0; w < 8; ++w) wt[w] = sw[(size_t)x * 8u + w];
            double v;
            if (match_five_planes(q.wcls | ((cm >> 8) & 15u))) v = match_score<MEASURE, 5>(s_q, wt, lc, q.P5, q.w0, lq);
            else v = match_score<MEASURE, 7>(s_q, wt, lc, q.P, q.w0, lq);
            const bool hit = need && match_join_hit(v, min_score, upper, i, j);
            if (FILL) {
                if (hit) join_store(cur, end, j, v, out_index, out_score);
            } else {
                count += hit ? 1u : 0u;
                if (__ballot(hit) != 0ull) bits |= bit;
            }
        }
        if (!FILL && at != ~0ull && lane0) wmap[at] = bits;
    }
    if (!FILL && have) cnt[(size_t)split * nq + i] = count; // (0 for a slow query: its hits are the fallback's)
}
