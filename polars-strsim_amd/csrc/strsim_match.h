// strsim_match.h -- best-match search: every row of a query column against a whole candidate column, the k best candidates
// per query (strsim_best_match_device).  Included by strsim_kernels.hip inside namespace strsim, after strsim_lane_lit.h.
//
//   k_match_pack        one thread per string: its bytes into eight registers' worth of words (zeros behind the string), its
//                       length and which of bits 5 / 6 its bytes take, or "slow" (longer than 32 bytes, non-ASCII) -- then the
//                       string's index goes to the slow list of its side.
//   k_match_lane<M, K>  ONE QUERY PER LANE, both strings <= 32 ASCII bytes.  The query's bit-planes are built once
//                       (match_lane_query, which the length-ordered sweep of strsim_nearest_kernels.h shares) and stay in
//                       registers for the whole sweep; the candidate is wave-uniform text, as the literal of k_lane_lit: its
//                       words, length and class come in through scalar loads and its per-column bit fills are scalar.  Each lane
//                       keeps its running top-K in VGPRs.  blockIdx.y splits the candidates; every split writes a partial
//                       top-K that k_match_merge reduces.
//   k_match_fold_cols   fallback, a slow QUERY against all candidates: the scores of strsim_pairs_device with the query as the
//                       literal, one workgroup per query -> its fallback top-K.
//   k_match_fold_rows   fallback, a slow CANDIDATE against all fast queries: the scores of strsim_pairs_device with the
//                       candidate as the literal, one thread per query -> the query's fallback top-K.
//   k_match_merge       the partial lists (+ the fallback list) of a query -> its first k slots; empty slots as (~0, NaN).
//
// Order of a list: descending score, ties to the lower candidate index (match_better).  Every insertion uses that one
// comparison, so the lists do not depend on the order in which candidates are seen.
#pragma once

constexpr int MATCH_BLOCK = 256;
constexpr uint32_t MATCH_SLOW = 0x80000000u; // meta: not in the lane class
constexpr uint32_t MATCH_NONE = 0xFFFFFFFFu; // empty slot

__device__ __forceinline__ bool match_better(double a, uint32_t ia, double b, uint32_t ib)
{
    return a > b || (a == b && ia < ib);
}

// (v, j) into a sorted list of K: one compare-and-swap per slot, fully unrolled (the slots stay in registers)
template <int K>
__device__ __forceinline__ void match_insert(double (&ts)[K], uint32_t (&ti)[K], double v, uint32_t j)
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const bool sw = match_better(v, j, ts[k], ti[k]);
        const double tv = ts[k];
        const uint32_t tj = ti[k];
        ts[k] = sw ? v : tv;
        ti[k] = sw ? j : tj;
        v = sw ? tv : v;
        j = sw ? tj : j;
    }
}

// meta of a string: length (bits 0..5), bit 8: some byte has bit 5 set, 9: some byte has it clear, 10 / 11: the same of bit 6;
// MATCH_SLOW for anything else.  Reads exactly the string's bytes.
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_pack(const uint32_t *__restrict__ off, const uint8_t *__restrict__ val,
                                                            uint32_t rows, uint32_t *__restrict__ words, uint32_t *__restrict__ meta,
                                                            uint32_t *__restrict__ slow_list, uint32_t *__restrict__ slow_count)
{
    const uint32_t i = blockIdx.x * MATCH_BLOCK + threadIdx.x;
    if (i >= rows) return;
    const uint32_t o0 = off[i], len = off[i + 1] - o0;
    uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t any = 0u, all = 0xFFu;
    bool slow = len > 32u;
    if (!slow) {
        for (uint32_t b = 0; b < len; ++b) {
            const uint32_t c = val[o0 + b];
            any |= c;
            all &= c;
            w[b >> 2] |= c << (8u * (b & 3u));
        }
        slow = (any & 0x80u) != 0u;
    }
    uint4 *const dst = reinterpret_cast<uint4 *>(words + (size_t)i * 8u);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    if (slow) {
        meta[i] = MATCH_SLOW;
        slow_list[atomicAdd(slow_count, 1u)] = i;
        return;
    }
    const uint32_t cls = (len ? ((any & 0x20u) ? 1u : 0u) | ((all & 0x20u) ? 0u : 2u) | ((any & 0x40u) ? 4u : 0u) |
                                    ((all & 0x40u) ? 0u : 8u)
                              : 0u);
    meta[i] = len | (cls << 8);
}

// bits 5 and 6 of every byte of the pair agree: five bit-planes separate the bytes (else seven; bit 7 is 0 in ASCII)
__device__ __forceinline__ bool match_five_planes(uint32_t cls)
{
    return (cls & 3u) != 3u && (cls & 12u) != 12u;
}

// The query of a lane as every sweep holds it (k_match_lane, search_sweep_lane): the bit-planes of query i's eight words (of
// zeros unless `live`), the first five of them again, the first word, and which values bits 5 / 6 take over the wave's live
// queries (uniform; qm is the query's meta).
struct LaneQuery {
    uint32_t P[7], P5[5], w0, wcls;
};
__device__ __forceinline__ LaneQuery match_lane_query(const uint32_t *__restrict__ qwords, uint32_t i, bool live, uint32_t qm)
{
    uint32_t wp[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (live) {
        const uint4 *const src = reinterpret_cast<const uint4 *>(qwords + (size_t)i * 8u);
        const uint4 a = src[0], b = src[1];
        wp[0] = a.x; wp[1] = a.y; wp[2] = a.z; wp[3] = a.w; wp[4] = b.x; wp[5] = b.y; wp[6] = b.z; wp[7] = b.w;
    }
    LaneQuery q;
    build_planes<7>(wp, q.P);
#pragma unroll
    for (int b = 0; b < 5; ++b) q.P5[b] = q.P[b];
    q.w0 = wp[0];
    q.wcls = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (__ballot(live && ((qm >> (8 + b)) & 1u))) q.wcls |= 1u << b;
    return q;
}

template <int MEASURE, int NP>
__device__ __forceinline__ double match_score(const double *q, const uint32_t (&wt)[8], uint32_t lt, const uint32_t (&P)[NP],
                                              uint32_t wp0, uint32_t lp)
{
    constexpr bool LEV = MEASURE == LEVENSHTEIN;
    constexpr bool JARO_LIKE = MEASURE == JARO || MEASURE == JARO_WINKLER;
    const uint32_t lp1 = lp ? lp : 1u;
    if (LEV) {
        // the codes of k_lane_lit: an empty candidate is 1.0 against an empty query, else 0.0 (strsim.rs:128, :160)
        uint32_t code;
        if (lt == 0u) code = lp == 0u ? 1u : (uint32_t)QTAB_N + 1u;
        else {
            const uint32_t dist = lit_lev_uniform_text<NP>(wt, lt, P, lp1);
            code = lp ? dist * (uint32_t)QTAB_N + (lt > lp ? lt : lp) : (uint32_t)QTAB_N + 1u;
        }
        return 1.0 - q[code];
    }
    uint32_t dist = 0u, m = 0u, t = 0u, isect = 0u;
    if (lt != 0u) { // (uniform)
        const uint32_t tmax = (lt + (uint32_t)COLS_PER_TEST - 1u) / (uint32_t)COLS_PER_TEST * (uint32_t)COLS_PER_TEST;
        lane_cores32<NP, false, JARO_LIKE, !JARO_LIKE>(wt, lt, lt, tmax, lp1, P, dist, m, t, isect);
    }
    if (JARO_LIKE) {
        const uint32_t pre = MEASURE == JARO_WINKLER && lt != 0u && lp != 0u ? common_prefix4(wt[0], lt, wp0, lp) : 0u;
        const uint32_t pk = m | (t << 6) | (lt << 12) | (lp << 18) | (pre << 24);
        const uint32_t h = t >> 1;
        return stage_epilogue<MEASURE>(pk, q[m * (uint32_t)QTAB_N + lt], q[m * (uint32_t)QTAB_N + lp],
                                       q[(m > h ? m - h : 0u) * (uint32_t)QTAB_N + m]);
    }
    return stage_epilogue<MEASURE>(isect | (lt << 6) | (lp << 12), 0.0, 0.0, 0.0);
}

// Grid: (ceil(nq / 256), splits).  Split s takes candidates [s * per, min(nc, (s + 1) * per)) and writes its top-K of every query to
// pscore / pidx[(s * nq + i) * K ..].
template <int MEASURE, int K>
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                            uint32_t nq, const uint32_t *__restrict__ cwords,
                                                            const uint32_t *__restrict__ cmeta, uint32_t nc, uint32_t per,
                                                            const double *__restrict__ qtab, double min_score,
                                                            double *__restrict__ pscore, uint32_t *__restrict__ pidx)
{
    constexpr bool TABLE = MEASURE == LEVENSHTEIN || MEASURE == JARO || MEASURE == JARO_WINKLER;
    __shared__ double s_q[TABLE ? QTAB_N * QTAB_N : 1];
    const uint32_t tid = threadIdx.x;
    if (TABLE)
        for (uint32_t x = tid; x < (uint32_t)(QTAB_N * QTAB_N); x += MATCH_BLOCK) s_q[x] = qtab[x];
    __syncthreads();

    const uint32_t i = blockIdx.x * MATCH_BLOCK + tid;
    const bool have = i < nq;
    const uint32_t qm = have ? qmeta[i] : MATCH_SLOW;
    const bool mine = (qm & MATCH_SLOW) == 0u;
    const uint32_t lp = qm & 63u;
    const LaneQuery q = match_lane_query(qwords, i, mine, qm);

    double ts[K];
    uint32_t ti[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { ts[k] = -__builtin_inf(); ti[k] = MATCH_NONE; }

    const uint32_t j0 = blockIdx.y * per;
    const uint32_t j1 = j0 >= nc ? j0 : (nc - j0 < per ? nc : j0 + per);
    if (__ballot(mine) != 0ull) {
        for (uint32_t j = j0; j < j1; ++j) { // (uniform: the candidate's words and meta are scalar loads)
            const uint32_t cm = cmeta[j];
            if (cm & MATCH_SLOW) continue;
            uint32_t wt[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) wt[q] = cwords[(size_t)j * 8u + q];
            const uint32_t lt = cm & 63u;
            double v;
            if (match_five_planes(q.wcls | ((cm >> 8) & 15u))) v = match_score<MEASURE, 5>(s_q, wt, lt, q.P5, q.w0, lp);
            else v = match_score<MEASURE, 7>(s_q, wt, lt, q.P, q.w0, lp);
            if (mine && v >= min_score && match_better(v, j, ts[K - 1], ti[K - 1])) match_insert<K>(ts, ti, v, j);
        }
    }
    if (!have) return;
    const size_t o = ((size_t)blockIdx.y * nq + i) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) { pscore[o + k] = ts[k]; pidx[o + k] = ti[k]; }
}

// Fill a list array with empty slots.
__global__ void k_match_clear(double *__restrict__ score, uint32_t *__restrict__ idx, uint64_t n)
{
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < n) { score[x] = -__builtin_inf(); idx[x] = MATCH_NONE; }
}

// Fallback: nb slow queries qlist[b], scores[b * nc + j] = score of (query qlist[b], candidate j).  One workgroup per query: each
// thread keeps the top-K of its strided candidates, K rounds of a workgroup arg-best pick the query's top-K, which is merged into
// its list (fscore / fidx[query * K ..]).
template <int K>
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_fold_cols(const double *__restrict__ scores, const uint32_t *__restrict__ qlist,
                                                                 uint32_t nc, double min_score, double *__restrict__ fscore,
                                                                 uint32_t *__restrict__ fidx)
{
    __shared__ double s_v[MATCH_BLOCK];
    __shared__ uint32_t s_j[MATCH_BLOCK];
    __shared__ double r_v[K];
    __shared__ uint32_t r_j[K];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const double *const row = scores + (size_t)b * nc;
    double ts[K];
    uint32_t ti[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { ts[k] = -__builtin_inf(); ti[k] = MATCH_NONE; }
    for (uint32_t j = tid; j < nc; j += MATCH_BLOCK) {
        const double v = row[j];
        if (v >= min_score && match_better(v, j, ts[K - 1], ti[K - 1])) match_insert<K>(ts, ti, v, j);
    }
    for (int r = 0; r < K; ++r) {
        s_v[tid] = ts[0];
        s_j[tid] = ti[0];
        __syncthreads();
        for (uint32_t h = MATCH_BLOCK / 2; h > 0; h >>= 1) {
            if (tid < h && match_better(s_v[tid + h], s_j[tid + h], s_v[tid], s_j[tid])) { s_v[tid] = s_v[tid + h]; s_j[tid] = s_j[tid + h]; }
            __syncthreads();
        }
        const uint32_t wj = s_j[0];
        if (tid == 0u) { r_v[r] = s_v[0]; r_j[r] = wj; }
        if (wj != MATCH_NONE && ti[0] == wj) { // the winner pops its head (candidate indices are distinct)
#pragma unroll
            for (int k = 0; k + 1 < K; ++k) { ts[k] = ts[k + 1]; ti[k] = ti[k + 1]; }
            ts[K - 1] = -__builtin_inf();
            ti[K - 1] = MATCH_NONE;
        }
        __syncthreads();
    }
    if (tid == 0u) {
        const size_t o = (size_t)qlist[b] * K;
        double fs[K];
        uint32_t fi[K];
#pragma unroll
        for (int k = 0; k < K; ++k) { fs[k] = fscore[o + k]; fi[k] = fidx[o + k]; }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (r_j[k] != MATCH_NONE) match_insert<K>(fs, fi, r_v[k], r_j[k]);
#pragma unroll
        for (int k = 0; k < K; ++k) { fscore[o + k] = fs[k]; fidx[o + k] = fi[k]; }
    }
}

// Fallback: nb slow candidates clist[b], scores[b * nq + i] = score of (query i, candidate clist[b]); slow queries are skipped
// (k_match_fold_cols saw all their candidates).  One thread per query.
template <int K>
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_fold_rows(const double *__restrict__ scores, const uint32_t *__restrict__ clist,
                                                                 uint32_t nb, const uint32_t *__restrict__ qmeta, uint32_t nq,
                                                                 double min_score, double *__restrict__ fscore, uint32_t *__restrict__ fidx)
{
    const uint32_t i = blockIdx.x * MATCH_BLOCK + threadIdx.x;
    if (i >= nq || (qmeta[i] & MATCH_SLOW)) return;
    const size_t o = (size_t)i * K;
    double fs[K];
    uint32_t fi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { fs[k] = fscore[o + k]; fi[k] = fidx[o + k]; }
    for (uint32_t b = 0; b < nb; ++b) {
        const double v = scores[(size_t)b * nq + i];
        const uint32_t j = clist[b];
        if (v >= min_score && match_better(v, j, fs[K - 1], fi[K - 1])) match_insert<K>(fs, fi, v, j);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) { fscore[o + k] = fs[k]; fidx[o + k] = fi[k]; }
}

// nl lists of K per query (list l of query i at (l * nq + i) * K) -> the query's first k slots; an empty slot is (~0, NaN).
template <int K>
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_merge(const double *__restrict__ pscore, const uint32_t *__restrict__ pidx,
                                                             uint32_t nl, uint32_t nq, uint32_t k, uint32_t *__restrict__ out_index,
                                                             double *__restrict__ out_score)
{
    const uint32_t i = blockIdx.x * MATCH_BLOCK + threadIdx.x;
    if (i >= nq) return;
    double ts[K];
    uint32_t ti[K];
#pragma unroll
    for (int s = 0; s < K; ++s) { ts[s] = -__builtin_inf(); ti[s] = MATCH_NONE; }
    for (uint32_t l = 0; l < nl; ++l) {
        const size_t o = ((size_t)l * nq + i) * K;
        for (int s = 0; s < K; ++s) { // (a list is sorted: the first entry that does not enter ends it)
            const uint32_t j = pidx[o + s];
            const double v = pscore[o + s];
            if (j == MATCH_NONE || !match_better(v, j, ts[K - 1], ti[K - 1])) break;
            match_insert<K>(ts, ti, v, j);
        }
    }
#pragma unroll
    for (int s = 0; s < K; ++s)
        if ((uint32_t)s < k) {
            out_index[(size_t)i * k + s] = ti[s];
            out_score[(size_t)i * k + s] = ti[s] == MATCH_NONE ? __builtin_nan("") : ts[s];
        }
}
