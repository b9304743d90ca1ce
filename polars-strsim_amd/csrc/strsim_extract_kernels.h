// strsim_extract_kernels.h -- the kernel of strsim_extract_device (the shared rules are in strsim_extract.h; DESIGN.md section
// 17).  Included by strsim_kernels.hip inside namespace strsim, after strsim_nearest_kernels.h: the strings are packed by
// k_match_pack, put in length order by k_nearest_hist / _scan / _scatter, the partial lists are reduced by k_match_merge and the
// fallback is folded by k_match_fold_cols / _rows.
//
//   k_extract_lane<K>   ONE QUERY PER LANE in length order, the query's bit-planes in registers, the candidate wave-uniform
//                       text read through scalar loads, the running top-K of (rank, j) in VGPRs as 64-bit keys.  The rank table
//                       (8.3 KB) is copied into LDS once per workgroup: a pair costs one LDS read instead of an f64 division.
//                       The wave sweeps the candidate lengths of its window nearest-first with the skip and stop rules of
//                       strsim_extract.h.  blockIdx.y takes its slice of every length bucket; the partial lists go to the
//                       query's original row with their f64 scores (epilogue_indel of the rank's representative pair).
#pragma once

// Grid and arguments as k_nearest_lane; rlimit >= 1 is the number of admissible ranks (extract_rank_limit).
template <int K>
__global__ __launch_bounds__(MATCH_BLOCK) void k_extract_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                              const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qstart,
                                                              uint32_t nq, const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                              const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ cstart,
                                                              const ExtractTable *__restrict__ tab, uint32_t rlimit,
                                                              double *__restrict__ pscore, uint32_t *__restrict__ pidx)
{
    __shared__ uint32_t s_words[EXTRACT_TAB_WORDS];
    {
        const uint32_t *const src = reinterpret_cast<const uint32_t *>(tab->rank);
        for (uint32_t x = threadIdx.x; x < EXTRACT_TAB_WORDS; x += MATCH_BLOCK) s_words[x] = src[x];
    }
    __syncthreads();
    const uint16_t *const s_rank = reinterpret_cast<const uint16_t *>(s_words);

    const uint32_t p = blockIdx.x * MATCH_BLOCK + threadIdx.x;
    const uint32_t split = blockIdx.y, splits = gridDim.y;
    const bool have = p < nq;
    const uint32_t i = have ? qperm[p] : 0u;
    const bool live = have && p < qstart[NEAREST_SLOW_BUCKET];
    const uint32_t qm = live ? qmeta[i] : 0u;
    const uint32_t lq = qm & 63u;
    uint32_t wp[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (live) {
        const uint4 *const src = reinterpret_cast<const uint4 *>(qwords + (size_t)i * 8u);
        const uint4 a = src[0], b = src[1];
        wp[0] = a.x; wp[1] = a.y; wp[2] = a.z; wp[3] = a.w; wp[4] = b.x; wp[5] = b.y; wp[6] = b.z; wp[7] = b.w;
    }
    uint32_t P[7];
    build_planes<7>(wp, P);
    const uint32_t P5[5] = {P[0], P[1], P[2], P[3], P[4]};
    // which values bits 5 / 6 take over the wave's queries (uniform)
    uint32_t wcls = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (__ballot(live && ((qm >> (8 + b)) & 1u))) wcls |= 1u << b;

    uint64_t keys[K];
#pragma unroll
    for (int s = 0; s < K; ++s) keys[s] = NEAREST_EMPTY;

    if (__ballot(live) != 0ull) {
        const uint32_t lmin = nearest_wave_min(live ? lq : 0xFFFFFFFFu), lmax = nearest_wave_max(live ? lq : 0u);
        uint32_t lo, hi;
        extract_window(s_rank, lmin, lmax, rlimit, lo, hi);
        const uint32_t steps = nearest_steps(lmin, lmax, lo, hi);
        for (uint32_t g = 0; g < steps; ++g) {
            uint32_t first, last, stride;
            if (!nearest_step_range(lmin, lmax, lo, hi, g, first, last, stride)) continue;
            bool needed = false; // (uniform) some live lane needs a length of this step
            for (uint32_t lc = first; lc <= last; lc += stride) {
                const uint32_t ubr = extract_ub(s_rank, lq, lc);
                const uint16_t *const row = s_rank + (lq + lc) * EXTRACT_TAB_W;
                if (__ballot(live && extract_needs(ubr, extract_bound(keys[K - 1], rlimit))) != 0ull) needed = true;
                // this split's slice of the bucket of length lc, while some lane still needs that length
                const uint32_t c0 = cstart[lc], n = cstart[lc + 1u] - c0;
                const uint32_t x1 = c0 + (uint32_t)((uint64_t)n * (split + 1u) / splits);
                for (uint32_t x = c0 + (uint32_t)((uint64_t)n * split / splits); x < x1; ++x) { // (uniform: scalar loads)
                    if (__ballot(live && extract_needs(ubr, extract_bound(keys[K - 1], rlimit))) == 0ull) break;
                    const uint32_t cm = sm[x], j = sidx[x];
                    uint32_t wt[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) wt[q] = sw[(size_t)x * 8u + q];
                    uint32_t d;
                    if (match_five_planes(wcls | ((cm >> 8) & 15u))) d = extract_indel_uniform_text<5>(wt, lc, P5, lq);
                    else d = extract_indel_uniform_text<7>(wt, lc, P, lq);
                    const uint32_t r = row[d]; // d <= lq + lc: inside the row
                    const uint64_t key = extract_key(r, j);
                    if (live && r < rlimit && key < keys[K - 1]) nearest_insert<K>(keys, key);
                }
            }
            if (!needed) break;
        }
    }
    if (!have) return;
    const size_t o = ((size_t)split * nq + i) * K;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        const bool e = keys[s] == NEAREST_EMPTY;
        const double v = extract_rank_score(tab->rep, e ? 0u : (uint32_t)(keys[s] >> 32)); // (an empty key has no rank)
        pscore[o + s] = e ? -__builtin_inf() : v;
        pidx[o + s] = e ? MATCH_NONE : (uint32_t)keys[s];
    }
}
