// strsim_cdist_kernels.h -- the kernels of strsim_cdist_device (the shared rules are in strsim_cdist.h).
// Included by strsim_kernels.hip inside namespace strsim, after strsim_extract_kernels.h: the strings are packed by k_match_pack.
//
//   k_cdist_lane<M>     k_match_lane's sweep without a list: ONE QUERY PER LANE, its bit-planes in registers, the candidate
//                       wave-uniform text through scalar loads, blockIdx.y splits the candidates.  Every score is kept: a wave
//                       stages 64 queries x CDIST_TJ candidates in a tile of LDS of its own (column-wise, one score per lane and
//                       candidate) and writes the tile out row-wise in 16-byte stores (cdist_item of strsim_cdist.h).  The tile
//                       is private to the wave: no workgroup barrier inside the candidate loop.  Measures 0 .. 4 score by
//                       match_score; Indel by extract_indel_uniform_text and one read of the [s][d] score table in LDS.  A pair
//                       with a side outside the lane class is written as 0.0; the fallback behind this grid overwrites it.
//   k_cdist_put_col     fallback, a slow CANDIDATE: a column of pairwise scores (one per query) into its column of the matrix;
//                       the rows of slow queries are left alone (their own pass wrote them).
//   k_cdist_cutoff      fallback, a slow QUERY: the cutoff rule over the rows the pairwise calls wrote.
#pragma once

template <int MEASURE>
__global__ __launch_bounds__(CDIST_BLOCK) void k_cdist_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                            uint32_t nq, const uint32_t *__restrict__ cwords,
                                                            const uint32_t *__restrict__ cmeta, uint32_t nc, uint32_t per,
                                                            const double *__restrict__ tab, double cutoff, double *__restrict__ out,
                                                            uint64_t ld)
{
    constexpr bool TABLE = MEASURE == LEVENSHTEIN || MEASURE == JARO || MEASURE == JARO_WINKLER || MEASURE == INDEL;
    static_assert(QTAB_N * QTAB_N == (int)CDIST_TAB_N, "the Indel score table takes the quotient table's place");
    __shared__ double s_q[TABLE ? QTAB_N * QTAB_N : 1];
    __shared__ double s_tile[CDIST_BLOCK / 64][CDIST_TILE];
    const uint32_t tid = threadIdx.x;
    if (TABLE)
        for (uint32_t x = tid; x < (uint32_t)(QTAB_N * QTAB_N); x += CDIST_BLOCK) s_q[x] = tab[x];
    __syncthreads();

    const uint32_t lane = tid & 63u;
    const uint32_t i0 = blockIdx.x * CDIST_BLOCK + (tid & ~63u); // the wave's first query
    if (i0 >= nq) return;                                         // (uniform; no workgroup barrier below)
    const uint32_t rows = nq - i0 < 64u ? nq - i0 : 64u;
    const uint32_t i = i0 + lane;
    const bool have = lane < rows;
    const uint32_t qm = have ? qmeta[i] : MATCH_SLOW;
    const bool mine = (qm & MATCH_SLOW) == 0u;
    const uint32_t lp = qm & 63u;
    const LaneQuery q = match_lane_query(qwords, i, mine, qm);
    const bool any = __ballot(mine) != 0ull;
    double *const tile = s_tile[tid >> 6];
    const uint64_t base8 = (uint64_t)reinterpret_cast<uintptr_t>(out) >> 3;

    uint32_t j0, j1;
    cdist_split_range(blockIdx.y, per, nc, j0, j1);
    for (uint32_t jt = j0; jt < j1; jt += CDIST_TJ) { // (uniform)
        const uint32_t n = j1 - jt < CDIST_TJ ? j1 - jt : CDIST_TJ;
        for (uint32_t jj = 0; jj < n; ++jj) {
            const uint32_t j = jt + jj;
            const uint32_t cm = cmeta[j];
            double v = 0.0;
            if (any && (cm & MATCH_SLOW) == 0u) { // (uniform: the candidate's words and meta are scalar loads)
                uint32_t wt[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) wt[w] = cwords[(size_t)j * 8u + w];
                const uint32_t lt = cm & 63u;
                const bool five = match_five_planes(q.wcls | ((cm >> 8) & 15u));
                if constexpr (MEASURE == INDEL) {
                    const uint32_t d = five ? extract_indel_uniform_text<5>(wt, lt, q.P5, lp) : extract_indel_uniform_text<7>(wt, lt, q.P, lp);
                    v = s_q[(lp + lt) * CDIST_TAB_W + d]; // d <= lp + lt <= 64
                } else {
                    v = five ? match_score<MEASURE, 5>(s_q, wt, lt, q.P5, q.w0, lp) : match_score<MEASURE, 7>(s_q, wt, lt, q.P, q.w0, lp);
                }
                v = mine ? cdist_cut(v, cutoff) : 0.0;
            }
            tile[cdist_tile_at(lane, jj)] = v;
        }
        // the wave's own LDS operations complete in order: the fences only keep the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (uint32_t pass = 0; pass < CDIST_PASSES; ++pass) {
            const CdistItem it = cdist_item(pass * 64u + lane, base8, i0, rows, ld, jt, n);
            if (it.count) {
                double *const dst = out + cdist_index((uint64_t)i0 + it.row, ld, (uint64_t)jt + it.col);
                const double a = tile[cdist_tile_at(it.row, it.col)];
                if (it.count == 2u) *reinterpret_cast<double2 *>(dst) = make_double2(a, tile[cdist_tile_at(it.row, it.col + 1u)]);
                else *dst = a;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// Grid (ceil(nq / 256), nb): scores[b * nq + i] = score of (query i, candidate clist[b]) -> out[i][clist[b]] under the cutoff.
__global__ __launch_bounds__(MATCH_BLOCK) void k_cdist_put_col(const double *__restrict__ scores, const uint32_t *__restrict__ clist,
                                                               const uint32_t *__restrict__ qmeta, uint32_t nq, double cutoff,
                                                               double *__restrict__ out, uint64_t ld)
{
    const uint32_t i = blockIdx.x * MATCH_BLOCK + threadIdx.x, b = blockIdx.y;
    if (i >= nq || (qmeta[i] & MATCH_SLOW)) return;
    out[cdist_index(i, ld, clist[b])] = cdist_cut(scores[(size_t)b * nq + i], cutoff);
}

// Grid (ceil(nc / 256), nb): the cutoff rule over row qlist[b] of the matrix.
__global__ __launch_bounds__(MATCH_BLOCK) void k_cdist_cutoff(double *__restrict__ out, const uint32_t *__restrict__ qlist, uint32_t nc,
                                                              uint64_t ld, double cutoff)
{
    const uint32_t j = blockIdx.x * MATCH_BLOCK + threadIdx.x;
    if (j >= nc) return;
    double *const p = out + cdist_index(qlist[blockIdx.y], ld, j);
    if (*p < cutoff) *p = 0.0;
}
