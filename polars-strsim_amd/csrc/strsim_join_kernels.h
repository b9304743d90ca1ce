// strsim_join_kernels.h -- the kernels of strsim_join_device (the shared rules are in strsim_join.h).
// Included by strsim_kernels.hip inside namespace strsim, after strsim_cdist_kernels.h: the strings are packed by k_match_pack and
// put in length order by k_nearest_hist / _scan / _scatter, once per call; both sweeps read that one order.
//
//   join_lane_start / join_lane_slice / join_lane_end   THE ONE BODY of a join's lane sweep, shared by k_join_lane and
//                       k_match_join_lane (strsim_match_join_kernels.h).  ONE QUERY PER LANE in length order, its bit-planes in
//                       registers (match_lane_query), the candidate wave-uniform text through scalar loads; blockIdx.y takes its
//                       slice of every length bucket.  FILL = false counts a lane's hits in a register and stores one count per
//                       (split, query), and marks in the wave's hit map which candidates had a hit at all; FILL = true computes those
//                       candidates only and stores (j, score) into the lane's own segment, the cursor compared with the segment's
//                       end before every store.  No atomics.  What a pair yields, whether it is a hit and the score that is stored
//                       come from the caller: a rule object (JoinRankRule, MatchJoinRule) with the kernel's own scoring call.
//   k_join_lane<FILL>   adds the rank table of strsim_extract.h in LDS and the visiting order: the lengths of the wave's window
//                       nearest-first, a length no live lane needs is skipped and the wave stops after a step none of whose lengths
//                       was needed (strsim_join.h).  A pair yields its rank; the f64 score is formed only on a hit that is stored
//                       (extract_rank_score).
//   k_join_totals       one thread per query: its counts into their exclusive prefix (join_row_prefix), the total to indptr[i + 1].
//   k_join_scan_sums / _top / _apply   the 64-bit inclusive scan of the totals in place: indptr.
//   k_join_slow<SIDE, FILL>  fallback.  SIDE 0: a slow QUERY's column of nc pairwise scores -> that row's hits; SIDE 1: a slow
//                       CANDIDATE's column of nq scores -> at most one hit of every fast query.  Counted into / stored in the
//                       query's fallback list; a position comes from an integer atomic cursor per row and is compared with the
//                       row's end before the store.
//   k_join_sort_rows<LONG>  every row's (j, score) pairs by j, the comparators of join_sort_pair.  LONG = false: one wave per row
//                       of 2 .. JOIN_SORT_WAVE_MAX hits, in LDS; LONG = true: one workgroup per longer row, in place in global
//                       memory, at any length.  Rows of 0 or 1 hits are skipped.
//
// Every loop is bounded by the kernel's arguments, no kernel waits on another workgroup, and every store is a plain vector store.
#pragma once

// The arguments both lane sweeps take, as the pieces below read them.  Grid: (ceil(nq / MATCH_BLOCK), splits); the queries and the
// length-ordered candidates of k_extract_lane, then: upper (STRSIM_JOIN_UPPER), cnt: (splits + 1) x nq words -- the counts (written
// by FILL = false), their prefix (read by FILL = true) --, the hit map (ceil(nq / 64) waves x map_words words, written by
// FILL = false, read by FILL = true; join_map_words / join_map_shift), indptr (FILL: nq + 1) and the outputs.
struct JoinSweep {
    const uint32_t *qwords, *qmeta, *qperm, *qstart; uint32_t nq;
    const uint32_t *sw, *sm, *sidx, *cstart;
    bool upper;
    uint32_t *cnt, *map; uint64_t map_words; uint32_t map_shift;
    const uint64_t *indptr; uint32_t *out_index; double *out_score;
};

// A lane of the sweep: its query, the wave's hit map and, between the slices, its count (FILL = false) or its cursor (FILL = true).
struct JoinLane {
    uint32_t split, splits;
    uint32_t i, lq;
    bool have, live;
    LaneQuery q;
    uint32_t *wmap; // the wave's hit map (strsim_join.h)
    bool lane0;
    uint32_t count;
    uint64_t cur, end; // FILL: the lane's segment (empty unless live)
};

template <bool FILL>
__device__ __forceinline__ void join_lane_start(const JoinSweep &s, JoinLane &L)
{
    // the last positions of the length order first: the longest queries have the widest windows and the longest candidates
    const uint32_t p = (gridDim.x - 1u - blockIdx.x) * MATCH_BLOCK + threadIdx.x;
    L.split = blockIdx.y, L.splits = gridDim.y;
    L.have = p < s.nq;
    L.i = L.have ? s.qperm[p] : 0u;
    L.live = L.have && p < s.qstart[NEAREST_SLOW_BUCKET];
    const uint32_t qm = L.live ? s.qmeta[L.i] : 0u;
    L.lq = qm & 63u;
    L.q = match_lane_query(s.qwords, L.i, L.live, qm);
    L.wmap = s.map + (size_t)(p >> 6) * s.map_words;
    L.lane0 = (threadIdx.x & 63u) == 0u;
    L.count = 0u;
    L.cur = 0u, L.end = 0u;
    if (FILL && L.live) {
        const uint64_t base = s.indptr[L.i];
        L.cur = base + s.cnt[(size_t)L.split * s.nq + L.i];
        L.end = base + s.cnt[(size_t)(L.split + 1u) * s.nq + L.i]; // (list `splits` is the fallback's: the row always exists)
    }
}

// One slice: the candidates of length lc that this split takes.  `need` is the lane's own (of (lq, lc) alone: out of the candidate
// loop); the caller has seen that some lane of the wave needs the length.  R.core<NP>(wt, lc, P, w0, lq, x) is the kernel's scoring call
// on this lane's planes and the candidate text wt (x: its position in the length order, uniform), R.value(c) what the pair yields, R.hit(v, upper, i, j) whether it is reported,
// R.score(v) the f64 that is stored.
template <bool FILL, class Rule>
__device__ __forceinline__ void join_lane_slice(const JoinSweep &s, JoinLane &L, uint32_t lc, bool need, const Rule &R)
{
    const uint32_t c0 = s.cstart[lc], n = s.cstart[lc + 1u] - c0;
    uint32_t x0, x1;
    join_slice(c0, n, L.split, L.splits, x0, x1);
    const uint32_t k = join_map_slice(lc, L.split, L.splits);
    uint64_t at = ~0ull; // the word of the hit map in hand (uniform), its bits
    uint32_t bits = 0u;
    for (uint32_t x = x0; x < x1; ++x) { // (uniform: scalar loads)
        const uint64_t w = join_map_word(x, s.map_shift, k);
        if (w != at) {
            if (!FILL && at != ~0ull && L.lane0) L.wmap[at] = bits;
            at = w;
            bits = FILL ? wave_uniform(L.wmap[w]) : 0u;
        }
        const uint32_t bit = join_map_bit(x, s.map_shift);
        if (FILL && !(bits & bit)) continue; // no lane of the wave had a hit in this group
        const uint32_t cm = s.sm[x], j = s.sidx[x];
        uint32_t wt[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) wt[w] = s.sw[(size_t)x * 8u + w];
        decltype(R.template core<5>(wt, lc, L.q.P5, L.q.w0, L.lq, x)) c;
        if (match_five_planes(L.q.wcls | ((cm >> 8) & 15u))) c = R.template core<5>(wt, lc, L.q.P5, L.q.w0, L.lq, x);
        else c = R.template core<7>(wt, lc, L.q.P, L.q.w0, L.lq, x);
        const auto v = R.value(c);
        const bool hit = need && R.hit(v, s.upper, L.i, j);
        if (FILL) {
            if (hit) join_store(L.cur, L.end, j, R.score(v), s.out_index, s.out_score);
        } else {
            L.count += hit ? 1u : 0u;
            if (__ballot(hit) != 0ull) bits |= bit;
        }
    }
    if (!FILL && at != ~0ull && L.lane0) L.wmap[at] = bits;
}

template <bool FILL>
__device__ __forceinline__ void join_lane_end(const JoinSweep &s, const JoinLane &L)
{
    if (!FILL && L.have) s.cnt[(size_t)L.split * s.nq + L.i] = L.count; // (0 for a slow query: its hits are the fallback's)
}

// JoinRankRule with the rank join's scoring call: the Indel distance of the pair.
struct JoinRankSweep : JoinRankRule {
    template <int NP>
    __device__ __forceinline__ uint32_t core(const uint32_t (&wt)[8], uint32_t lc, const uint32_t (&P)[NP], uint32_t, uint32_t lq, uint32_t) const
    {
        return extract_indel_uniform_text<NP>(wt, lc, P, lq);
    }
};

// The sweep of JoinSweep's arguments over the rank table `tab` under the integer cutoff rlimit >= 1.
template <bool FILL>
__global__ __launch_bounds__(MATCH_BLOCK) void k_join_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                           const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qstart,
                                                           uint32_t nq, const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                           const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ cstart,
                                                           const ExtractTable *__restrict__ tab, uint32_t rlimit, uint32_t upper_flag,
                                                           uint32_t *__restrict__ cnt, uint32_t *__restrict__ map, uint64_t map_words,
                                                           uint32_t map_shift, const uint64_t *__restrict__ indptr,
                                                           uint32_t *__restrict__ out_index, double *__restrict__ out_score)
{
    __shared__ uint32_t s_words[EXTRACT_TAB_WORDS];
    {
        const uint32_t *const src = reinterpret_cast<const uint32_t *>(tab->rank);
        for (uint32_t x = threadIdx.x; x < EXTRACT_TAB_WORDS; x += MATCH_BLOCK) s_words[x] = src[x];
    }
    __syncthreads();
    const uint16_t *const s_rank = reinterpret_cast<const uint16_t *>(s_words);

    const JoinSweep s{qwords, qmeta, qperm, qstart, nq, sw, sm, sidx, cstart, upper_flag != 0u, cnt, map, map_words, map_shift, indptr,
                      out_index, out_score};
    JoinLane L;
    join_lane_start<FILL>(s, L);
    if (__ballot(L.live) != 0ull) {
        const uint32_t lmin = nearest_wave_min(L.live ? L.lq : 0xFFFFFFFFu), lmax = nearest_wave_max(L.live ? L.lq : 0u);
        uint32_t lo, hi;
        extract_window(s_rank, lmin, lmax, rlimit, lo, hi);
        const uint32_t steps = nearest_steps(lmin, lmax, lo, hi);
        for (uint32_t g = 0; g < steps; ++g) {
            uint32_t first, last, stride;
            if (!nearest_step_range(lmin, lmax, lo, hi, g, first, last, stride)) continue;
            bool needed = false; // (uniform) some live lane needs a length of this step
            for (uint32_t lc = first; lc <= last; lc += stride) {
                const bool need = L.live && join_needs(s_rank, L.lq, lc, rlimit);
                if (__ballot(need) == 0ull) continue;
                needed = true;
                const JoinRankSweep R{{s_rank + (L.lq + lc) * EXTRACT_TAB_W, rlimit, tab->rep}};
                join_lane_slice<FILL>(s, L, lc, need, R);
            }
            if (!needed) break;
        }
    }
    join_lane_end<FILL>(s, L);
}

// One thread per query: cnt[l * nq + i], l < lists, into their exclusive prefix; indptr[i + 1] = the row's total, indptr[0] = 0.
__global__ __launch_bounds__(MATCH_BLOCK) void k_join_totals(uint32_t *__restrict__ cnt, uint32_t nq, uint32_t lists, uint64_t *__restrict__ indptr)
{
    const uint32_t i = blockIdx.x * MATCH_BLOCK + threadIdx.x;
    if (i == 0u) indptr[0] = 0u;
    if (i < nq) indptr[(size_t)i + 1u] = join_row_prefix(cnt, nq, i, lists);
}

// The exclusive scan of a workgroup's JOIN_SCAN_BLOCK thread sums in LDS; returns the thread's base, *total the workgroup's sum.
__device__ __forceinline__ uint64_t join_block_exclusive(uint64_t mine, uint64_t *s, uint64_t *total)
{
    const uint32_t tid = threadIdx.x;
    s[tid] = mine;
    __syncthreads();
    for (uint32_t h = 1u; h < JOIN_SCAN_BLOCK; h <<= 1) {
        const uint64_t add = tid >= h ? s[tid - h] : 0u;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const uint64_t incl = s[tid];
    if (total) *total = s[JOIN_SCAN_BLOCK - 1u];
    return incl - mine;
}

// Grid: join_scan_blocks(n).  sums[b] = the sum of workgroup b's values.
__global__ __launch_bounds__(JOIN_SCAN_BLOCK) void k_join_scan_sums(const uint64_t *__restrict__ v, uint64_t n, uint64_t *__restrict__ sums)
{
    __shared__ uint64_t s[JOIN_SCAN_BLOCK];
    uint64_t first, last, total;
    join_scan_range(blockIdx.x, threadIdx.x, n, first, last);
    join_block_exclusive(join_scan_sum(v, first, last), s, &total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}

// One workgroup: sums[0 .. nb) into their exclusive scan.
__global__ __launch_bounds__(JOIN_SCAN_BLOCK) void k_join_scan_top(uint64_t *__restrict__ sums, uint64_t nb)
{
    __shared__ uint64_t s[JOIN_SCAN_BLOCK];
    uint64_t first, last;
    join_scan_top_range(threadIdx.x, nb, first, last);
    uint64_t base = join_block_exclusive(join_scan_sum(sums, first, last), s, nullptr);
    for (uint64_t x = first; x < last; ++x) {
        const uint64_t t = sums[x];
        sums[x] = base;
        base += t;
    }
}

// Grid: join_scan_blocks(n).  v into its inclusive scan, workgroup b on top of sums[b].
__global__ __launch_bounds__(JOIN_SCAN_BLOCK) void k_join_scan_apply(uint64_t *__restrict__ v, uint64_t n, const uint64_t *__restrict__ sums)
{
    __shared__ uint64_t s[JOIN_SCAN_BLOCK];
    uint64_t first, last;
    join_scan_range(blockIdx.x, threadIdx.x, n, first, last);
    const uint64_t base = join_block_exclusive(join_scan_sum(v, first, last), s, nullptr);
    join_scan_write(v, first, last, sums[blockIdx.x] + base);
}

// Grid (ceil(rows / 256), nb), rows = nc (SIDE 0) or nq (SIDE 1): scores[b * rows + x] is the pairwise score of slow string
// list[b] against string x of the other side.  fb: the fallback's list of the counts, nq words (FILL: its prefix); cur: nq
// cursors, zeroed before the fill.
template <int SIDE, bool FILL>
__global__ __launch_bounds__(MATCH_BLOCK) void k_join_slow(const double *__restrict__ scores, const uint32_t *__restrict__ list,
                                                           const uint32_t *__restrict__ qmeta, uint32_t rows, double cutoff, uint32_t upper,
                                                           uint32_t *__restrict__ fb, uint32_t *__restrict__ cur,
                                                           const uint64_t *__restrict__ indptr, uint32_t *__restrict__ out_index,
                                                           double *__restrict__ out_score)
{
    const uint32_t x = blockIdx.x * MATCH_BLOCK + threadIdx.x, b = blockIdx.y;
    if (x >= rows) return;
    const uint32_t i = SIDE == 0 ? list[b] : x, j = SIDE == 0 ? x : list[b];
    if (SIDE == 1 && (qmeta[i] & MATCH_SLOW)) return; // (a slow query's own pass has the pair)
    const double v = scores[(size_t)b * rows + x];
    if (!(v >= cutoff) || (upper && j <= i)) return;
    if (!FILL) {
        atomicAdd(&fb[i], 1u);
        return;
    }
    uint64_t at = indptr[i] + fb[i] + atomicAdd(&cur[i], 1u);
    join_store(at, indptr[(size_t)i + 1u], j, v, out_index, out_score);
}

// LONG = false: grid ceil(nq / 4) workgroups of four waves, wave w of workgroup g sorts row 4 g + w when it has 2 ..
// JOIN_SORT_WAVE_MAX hits, in LDS of its own (no workgroup barrier).  LONG = true: workgroup g sorts rows g, g + gridDim.x, ..
// that have more hits, in place (the row's length is uniform over the workgroup: so is every barrier).
template <bool LONG>
__global__ __launch_bounds__(JOIN_SORT_BLOCK) void k_join_sort_rows(const uint64_t *__restrict__ indptr, uint32_t nq, uint32_t *index, double *score)
{
    if constexpr (LONG) {
        for (uint32_t i = blockIdx.x; i < nq; i += gridDim.x) {
            const uint64_t r0 = indptr[i], n = indptr[(size_t)i + 1u] - r0;
            if (n <= JOIN_SORT_WAVE_MAX) continue;
            uint32_t *const ri = index + r0;
            double *const rs = score + r0;
            const uint64_t P = join_sort_pow2(n);
            for (uint64_t k = 2u; k <= P; k <<= 1)
                for (uint64_t h = k >> 1; h > 0u; h >>= 1) {
                    for (uint64_t t = threadIdx.x; t < P / 2u; t += JOIN_SORT_BLOCK) {
                        uint64_t ca, cb;
                        join_sort_pair(t, k, h, ca, cb);
                        if (cb < n) join_sort_cmpx(ri, rs, ca, cb);
                    }
                    __syncthreads();
                }
        }
    } else {
        __shared__ uint32_t s_i[JOIN_SORT_BLOCK / 64u][JOIN_SORT_WAVE_MAX];
        __shared__ double s_s[JOIN_SORT_BLOCK / 64u][JOIN_SORT_WAVE_MAX];
        const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
        const uint64_t i = (uint64_t)blockIdx.x * (JOIN_SORT_BLOCK / 64u) + wave;
        if (i >= nq) return; // (uniform over the wave; no workgroup barrier below)
        const uint64_t r0 = indptr[i], n64 = indptr[i + 1u] - r0;
        if (n64 < 2u || n64 > JOIN_SORT_WAVE_MAX) return;
        const uint32_t n = (uint32_t)n64;
        uint32_t *const li = s_i[wave];
        double *const ls = s_s[wave];
        for (uint32_t x = lane; x < n; x += 64u) { li[x] = index[r0 + x]; ls[x] = score[r0 + x]; }
        const uint32_t P = (uint32_t)join_sort_pow2(n);
        for (uint32_t k = 2u; k <= P; k <<= 1)
            for (uint32_t h = k >> 1; h > 0u; h >>= 1) {
                // the wave's own LDS operations complete in order: the fences only keep the compiler from moving them
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (uint32_t t = lane; t < P / 2u; t += 64u) {
                    uint64_t ca, cb;
                    join_sort_pair(t, k, h, ca, cb);
                    if (cb < n) join_sort_cmpx(li, ls, ca, cb);
                }
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t x = lane; x < n; x += 64u) { index[r0 + x] = li[x]; score[r0 + x] = ls[x]; }
    }
}
