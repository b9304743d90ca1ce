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
//   search_sweep_lane<Rules, K>  the body of the two length-ordered lane kernels (k_nearest_lane here, k_extract_lane in
//                       strsim_extract_kernels.h): ONE QUERY PER LANE in length order, the query's bit-planes in registers, the
//                       candidate wave-uniform text read through scalar loads, the running top-K in VGPRs as 64-bit keys.  The
//                       wave sweeps the candidate lengths of its window nearest-first with the skip and stop rules of its Rules.
//                       blockIdx.y takes its slice of every length bucket; the partial lists go to the query's original row.
//   k_nearest_lane<TR, K>  that sweep under NearestRules<TR> (strsim_nearest.h): keys (d, j).
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

// The sweep of the length-ordered searches, written once: k_nearest_lane runs it with NearestRules (strsim_nearest.h) and
// k_extract_lane (strsim_extract_kernels.h) with ExtractRules (strsim_extract.h) -- one sweep, two rule sets.  Rules supplies the
// window, the value a lane keeps per candidate length (at), the skip test (needs), the distance core, the key of a pair and the
// f64 score of a kept key; the stop rule is chosen at compile time by Rules::STOP_BY_BOUND.  What is here is the loop and its wave
// operations (the ballots and the wave minimum / maximum); tests/cpu_harness/sweep_host.h is the same loop on the host.
//
// Grid: (ceil(nq / MATCH_BLOCK), splits).  Position p of the query permutation (qstart[NEAREST_SLOW_BUCKET] fast queries in
// length order, the slow ones behind them) writes the partial list of split blockIdx.y for its query i: pscore / pidx[(y * nq +
// i) * K ..], empty for a slow query.  Split y takes [c0 + n * y / splits, c0 + n * (y + 1) / splits) of every length bucket
// [c0, c0 + n) of the length-ordered candidates (sw / sm / sidx, bucket starts in cstart).
template <class Rules, int K>
__device__ __forceinline__ void search_sweep_lane(const Rules &R, const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                  const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qstart, uint32_t nq,
                                                  const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                  const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ cstart,
                                                  double *__restrict__ pscore, uint32_t *__restrict__ pidx)
{
    const uint32_t p = blockIdx.x * MATCH_BLOCK + threadIdx.x;
    const uint32_t split = blockIdx.y, splits = gridDim.y;
    const bool have = p < nq;
    const uint32_t i = have ? qperm[p] : 0u;
    const bool live = have && p < qstart[NEAREST_SLOW_BUCKET];
    const uint32_t qm = live ? qmeta[i] : 0u;
    const uint32_t lq = qm & 63u;
    const LaneQuery q = match_lane_query(qwords, i, live, qm);

    uint64_t keys[K];
#pragma unroll
    for (int s = 0; s < K; ++s) keys[s] = NEAREST_EMPTY;

    if (__ballot(live) != 0ull) {
        const uint32_t lmin = nearest_wave_min(live ? lq : 0xFFFFFFFFu), lmax = nearest_wave_max(live ? lq : 0u);
        uint32_t lo, hi;
        R.window(lmin, lmax, lo, hi);
        const uint32_t steps = nearest_steps(lmin, lmax, lo, hi);
        for (uint32_t g = 0; g < steps; ++g) {
            if constexpr (Rules::STOP_BY_BOUND)
                if (g && R.done(g, nearest_wave_max(live ? R.bound(keys[K - 1]) : 0u))) break;
            uint32_t first, last, stride;
            if (!nearest_step_range(lmin, lmax, lo, hi, g, first, last, stride)) continue;
            [[maybe_unused]] bool needed = false; // (uniform) some live lane needs a length of this step
            for (uint32_t lc = first; lc <= last; lc += stride) {
                const auto len = R.at(lq, lc);
                if constexpr (!Rules::STOP_BY_BOUND)
                    if (__ballot(live && R.needs(lq, len, keys[K - 1])) != 0ull) needed = true;
                // this split's slice of the bucket of length lc, while some lane still needs that length
                const uint32_t c0 = cstart[lc], n = cstart[lc + 1u] - c0;
                const uint32_t x1 = c0 + (uint32_t)((uint64_t)n * (split + 1u) / splits);
                for (uint32_t x = c0 + (uint32_t)((uint64_t)n * split / splits); x < x1; ++x) { // (uniform: scalar loads)
                    if (__ballot(live && R.needs(lq, len, keys[K - 1])) == 0ull) break;
                    const uint32_t cm = sm[x], j = sidx[x];
                    uint32_t wt[8];
#pragma unroll
                    for (int w = 0; w < 8; ++w) wt[w] = sw[(size_t)x * 8u + w];
                    uint32_t d;
                    if (match_five_planes(q.wcls | ((cm >> 8) & 15u))) d = R.template distance<5>(wt, lc, q.P5, lq);
                    else d = R.template distance<7>(wt, lc, q.P, lq);
                    bool ok;
                    const uint64_t key = R.key(d, len, j, ok);
                    if (live && ok && key < keys[K - 1]) nearest_insert<K>(keys, key);
                }
            }
            if constexpr (!Rules::STOP_BY_BOUND)
                if (!needed) break;
        }
    }
    if (!have) return;
    const size_t o = ((size_t)split * nq + i) * K;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        const bool e = keys[s] == NEAREST_EMPTY;
        const double v = R.score(e ? 0ull : keys[s]); // (an empty key has no score)
        pscore[o + s] = e ? -__builtin_inf() : v;
        pidx[o + s] = e ? MATCH_NONE : (uint32_t)keys[s];
    }
}

// search_sweep_lane under NearestRules<TR>: the partial lists carry the score -(double)d.
template <bool TR, int K>
__global__ __launch_bounds__(MATCH_BLOCK) void k_nearest_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                              const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qstart,
                                                              uint32_t nq, const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                              const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ cstart,
                                                              uint32_t kmax, double *__restrict__ pscore, uint32_t *__restrict__ pidx)
{
    search_sweep_lane<NearestRules<TR>, K>(NearestRules<TR>{kmax}, qwords, qmeta, qperm, qstart, nq, sw, sm, sidx, cstart, pscore, pidx);
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
