// strsim_nearest_kernels.h -- the kernels of strsim_nearest_device (the shared rules are in strsim_nearest.h; DESIGN.md section
// 13).  Included by strsim_kernels.hip inside namespace strsim, after strsim_match.h: the strings are packed by k_match_pack, the
// partial lists are reduced by k_match_merge and the fallback is folded by k_match_fold_cols / _rows, with a list entry (d, j)
// carried as the score -(double)d (match_better's order on it is ascending d, ties to the lower index).
//
//   k_nearest_hist      one thread per string: the histogram of one side's length buckets (0..32, slow strings in bucket 33).
//   k_nearest_scan      one thread: both histograms -> the start of every bucket, and the cursors of the scatter.
//   k_nearest_scatter   one thread per string: its position in length order (a workgroup claims a range of each bucket, its
//                       strings take their places in it by an LDS atomic, so the order inside a bucket varies from run to run).
//                       Queries: the permutation (the slow ones at the end).  Candidates: words, meta and original index,
//                       copied into length order so that a sweep reads them contiguously.
//   k_nearest_lane<TR, K>  ONE QUERY PER LANE in length order, the query's bit-planes in registers, the candidate wave-uniform
//                       text read through scalar loads, the running top-K of (d, j) in VGPRs as 64-bit keys.  The wave sweeps
//                       the candidate lengths of its window nearest-first with the skip and stop rules of strsim_nearest.h.
//                       blockIdx.y takes its slice of every length bucket; the partial lists go to the query's original row.
//   k_nearest_scores    fallback distances (uint32) -> the scores the fold kernels take.
//   k_nearest_finish    the merged scores -> distances, 0xFFFFFFFF in an empty slot.
#pragma once

__global__ __launch_bounds__(MATCH_BLOCK) void k_nearest_hist(const uint32_t *__restrict__ meta, uint32_t rows, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_h[NEAREST_BUCKETS];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * MATCH_BLOCK + tid;
    if (tid < NEAREST_BUCKETS) s_h[tid] = 0u;
    __syncthreads();
    if (i < rows) {
        const uint32_t m = meta[i];
        atomicAdd(&s_h[(m & MATCH_SLOW) ? NEAREST_SLOW_BUCKET : (m & 63u)], 1u);
    }
    __syncthreads();
    if (tid < NEAREST_BUCKETS && s_h[tid]) atomicAdd(&hist[tid], s_h[tid]);
}

// start[b] = the first position of bucket b (start[NEAREST_BUCKETS] = rows); cursor[b] = start[b]
__global__ void k_nearest_scan(const uint32_t *__restrict__ qhist, const uint32_t *__restrict__ chist, uint32_t *__restrict__ qstart,
                               uint32_t *__restrict__ cstart, uint32_t *__restrict__ qcur, uint32_t *__restrict__ ccur)
{
    if (threadIdx.x != 0u) return;
    uint32_t qa = 0u, ca = 0u;
    for (uint32_t b = 0; b < NEAREST_BUCKETS; ++b) {
        qstart[b] = qa; qcur[b] = qa; qa += qhist[b];
        cstart[b] = ca; ccur[b] = ca; ca += chist[b];
    }
    qstart[NEAREST_BUCKETS] = qa;
    cstart[NEAREST_BUCKETS] = ca;
}

// CAND = 0: perm[pos] = i for every query.  CAND = 1: the fast candidates' words / meta / index at their position.
template <int CAND>
__global__ __launch_bounds__(MATCH_BLOCK) void k_nearest_scatter(const uint32_t *__restrict__ words, const uint32_t *__restrict__ meta,
                                                                 uint32_t rows, uint32_t *__restrict__ cursor, uint32_t *__restrict__ perm,
                                                                 uint32_t *__restrict__ swords, uint32_t *__restrict__ smeta)
{
    __shared__ uint32_t s_n[NEAREST_BUCKETS], s_base[NEAREST_BUCKETS];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * MATCH_BLOCK + tid;
    if (tid < NEAREST_BUCKETS) s_n[tid] = 0u;
    __syncthreads();
    const uint32_t m = i < rows ? meta[i] : MATCH_SLOW;
    const uint32_t b = (m & MATCH_SLOW) ? NEAREST_SLOW_BUCKET : (m & 63u);
    const bool take = i < rows && (CAND == 0 || b != NEAREST_SLOW_BUCKET);
    const uint32_t r = take ? atomicAdd(&s_n[b], 1u) : 0u;
    __syncthreads();
    if (tid < NEAREST_BUCKETS && s_n[tid]) s_base[tid] = atomicAdd(&cursor[tid], s_n[tid]);
    __syncthreads();
    if (!take) return;
    const uint32_t pos = s_base[b] + r;
    perm[pos] = i;
    if (CAND) {
        const uint4 *const src = reinterpret_cast<const uint4 *>(words + (size_t)i * 8u);
        uint4 *const dst = reinterpret_cast<uint4 *>(swords + (size_t)pos * 8u);
        dst[0] = src[0];
        dst[1] = src[1];
        smeta[pos] = m;
    }
}

__device__ __forceinline__ uint32_t nearest_wave_min(uint32_t v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, s, 64);
        v = o < v ? o : v;
    }
    return wave_uniform(v);
}

__device__ __forceinline__ uint32_t nearest_wave_max(uint32_t v) { return wave_uniform(osa_wave_max(v)); }

// d of the lane's query (planes P, length lq) against the uniform candidate text wt of length lt
template <bool TR, int NP>
__device__ __forceinline__ uint32_t nearest_distance(const uint32_t (&wt)[8], uint32_t lt, const uint32_t (&P)[NP], uint32_t lq)
{
    return TR ? nearest_osa_uniform_text<NP>(wt, lt, P, lq) : nearest_lev_uniform_text<NP>(wt, lt, P, lq);
}

// Grid: (ceil(nq / MATCH_BLOCK), splits).  Position p of the query permutation (qstart[NEAREST_SLOW_BUCKET] fast queries in
// length order, the slow ones behind them) writes the partial list of split blockIdx.y for its query i: pscore / pidx[(y * nq +
// i) * K ..], empty for a slow query.  Split y takes [c0 + n * y / splits, c0 + n * (y + 1) / splits) of every length bucket
// [c0, c0 + n) of the length-ordered candidates (sw / sm / sidx, bucket starts in cstart).
template <bool TR, int K>
__global__ __launch_bounds__(MATCH_BLOCK) void k_nearest_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                              const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qstart,
                                                              uint32_t nq, const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                              const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ cstart,
                                                              uint32_t kmax, double *__restrict__ pscore, uint32_t *__restrict__ pidx)
{
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
        nearest_window(lmin, lmax, kmax, lo, hi);
        const uint32_t steps = nearest_steps(lmin, lmax, lo, hi);
        for (uint32_t g = 0; g < steps; ++g) {
            if (g && nearest_done(g, nearest_wave_max(live ? nearest_bound(keys[K - 1], kmax) : 0u))) break;
            uint32_t first, last, stride;
            if (!nearest_step_range(lmin, lmax, lo, hi, g, first, last, stride)) continue;
            for (uint32_t lc = first; lc <= last; lc += stride) {
                // this split's slice of the bucket of length lc, while some lane still needs that length
                const uint32_t c0 = cstart[lc], n = cstart[lc + 1u] - c0;
                const uint32_t x1 = c0 + (uint32_t)((uint64_t)n * (split + 1u) / splits);
                for (uint32_t x = c0 + (uint32_t)((uint64_t)n * split / splits); x < x1; ++x) { // (uniform: scalar loads)
                    if (__ballot(live && nearest_needs(lq, lc, nearest_bound(keys[K - 1], kmax))) == 0ull) break;
                    const uint32_t cm = sm[x], j = sidx[x];
                    uint32_t wt[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) wt[q] = sw[(size_t)x * 8u + q];
                    uint32_t d;
                    if (match_five_planes(wcls | ((cm >> 8) & 15u))) d = nearest_distance<TR, 5>(wt, lc, P5, lq);
                    else d = nearest_distance<TR, 7>(wt, lc, P, lq);
                    const uint64_t key = nearest_key(d, j);
                    if (live && d <= kmax && key < keys[K - 1]) nearest_insert<K>(keys, key);
                }
            }
        }
    }
    if (!have) return;
    const size_t o = ((size_t)split * nq + i) * K;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        const bool e = keys[s] == NEAREST_EMPTY;
        pscore[o + s] = e ? -__builtin_inf() : -(double)(uint32_t)(keys[s] >> 32);
        pidx[o + s] = e ? MATCH_NONE : (uint32_t)keys[s];
    }
}

__global__ __launch_bounds__(MATCH_BLOCK) void k_nearest_scores(const uint32_t *__restrict__ dist, uint64_t n, double *__restrict__ score)
{
    const uint64_t x = (uint64_t)blockIdx.x * MATCH_BLOCK + threadIdx.x;
    if (x < n) score[x] = -(double)dist[x];
}

__global__ __launch_bounds__(MATCH_BLOCK) void k_nearest_finish(const double *__restrict__ score, const uint32_t *__restrict__ index,
                                                                uint64_t n, uint32_t *__restrict__ dist)
{
    const uint64_t x = (uint64_t)blockIdx.x * MATCH_BLOCK + threadIdx.x;
    if (x < n) dist[x] = index[x] == MATCH_NONE ? MATCH_NONE : (uint32_t)(-score[x]);
}
