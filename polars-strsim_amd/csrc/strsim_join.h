// strsim_join.h -- threshold join: every pair (query i, candidate j) with score(i, j) >= score_cutoff, as CSR in ascending
// candidate index (strsim_join_device; record linkage and deduplication: "which pairs score at least 0.85").
// score = indel(q, c) of strsim_indel.h, bit for bit the pairwise call's; STRSIM_JOIN_UPPER keeps only j > i (a self-join).
//
// This header holds what the host shares with the kernels (tests/cpu_harness/join_sweep_host.h and join_harness.cpp compile it with
// g++): the skip and hit rules of a wave's sweep and the rule object that carries them into the sweep's one body (JoinRankRule),
// the slice a split takes of a length bucket, the split rule, the layout of the per-(list, query) counts and their prefix, the hit
// map, the 64-bit scan's partition and the comparators of the row sort.  The kernels are in strsim_join_kernels.h; the body of the
// sweep there (join_lane_start / _slice / _end) is also strsim_match_join.h's, under a rule object of its own.
//
// Two sweeps, no lists.  The queries and candidates of the lane class (at most 32 ASCII bytes) are put in length order once per
// call (k_match_pack, k_nearest_hist / _scan / _scatter) and swept twice by k_join_lane over the rank table of strsim_extract.h,
// where the cutoff is the integer rlimit: a pair is a hit iff rank[lq + lc][d] < rlimit.
//   - count: every lane counts its hits in a register and stores one count per (split, query): cnt[split * nq + i];
//   - the counts of a query (its splits, then one more list: the fallback's) become their exclusive prefix in place, their total
//     goes through a 64-bit scan into indptr, and nnz = indptr[nq] is read back;
//   - fill (only when nnz <= capacity): the same sweep over the same order, computing only the candidates the count sweep marked in
//     its hit map (below), stores (j, score) from indptr[i] + cnt[split * nq + i]
//     on and never at or beyond indptr[i] + cnt[(split + 1) * nq + i] -- the cursor is compared with that end before every store,
//     so whatever a sweep does, a store lands inside the segment the counts gave it, and the segments partition [0, nnz);
//   - the rows are then sorted by candidate index (k_join_sort_rows): the order in which a sweep meets candidates depends on the
//     length order and the splits, the result does not.
//
// Pruning (exact, the argument of strsim_extract.h without a top-k bound).  d >= |lq - lc|, so no candidate of length lc ranks
// better than ub(lq, lc) = rank[lq + lc][|lq - lc|], and a lane needs length lc iff ub(lq, lc) < rlimit: a function of (lq, lc)
// alone, taken out of the candidate loop.  The wave visits the lengths of extract_window(lmin, lmax, rlimit) nearest-first
// (nearest_step_range), skips a length no live lane needs (a ballot) and stops after a step none of whose lengths was needed: ub
// only worsens on the way out, so no later step holds a hit.
//
// Strings outside the lane class go through strsim_pairs_device(STRSIM_INDEL) with that string as the literal, as in cdist: a slow
// query's column of c_rows scores gives that row's hits, a slow candidate's column of q_rows scores adds at most one hit to every
// fast query.  These hits are counted and stored in the query's last list (the fallback's) at positions an integer cursor per row
// hands out; the row sort puts them in place.  The score columns of the count pass are kept for the fill when they fit
// JOIN_KEEP_SCORES doubles; beyond that BOTH passes run the pairwise calls.
#pragma once
#include <stdint.h>

#include "strsim_extract.h"

namespace strsim {

constexpr uint32_t JOIN_UPPER = 1u;           // STRSIM_JOIN_UPPER
constexpr uint32_t JOIN_MAX_SPLITS = 64u;     // grid.y of k_join_lane at most: (splits + 1) counts per query
constexpr uint32_t JOIN_MIN_PER_SPLIT = 64u;  // candidates per split at least
constexpr uint64_t JOIN_KEEP_SCORES = (uint64_t)1 << 24; // fallback scores kept from the count pass for the fill at most (128 MB)
constexpr uint32_t JOIN_SORT_WAVE_MAX = 512u; // tier limit of k_join_sort_rows: a row of up to this many hits is sorted by one wave in LDS
constexpr uint32_t JOIN_SORT_BLOCK = 256u;    // threads of a workgroup of k_join_sort_rows
constexpr uint32_t JOIN_SCAN_BLOCK = 256u;    // threads of a workgroup of the 64-bit scan
constexpr uint32_t JOIN_SCAN_PER = 8u;        // consecutive values per thread
constexpr uint32_t JOIN_SCAN_TILE = JOIN_SCAN_BLOCK * JOIN_SCAN_PER;

// Whether a query of length lq can have a hit among the candidates of length lc under rlimit >= 1.
STRSIM_HD bool join_needs(const uint16_t *rank, uint32_t lq, uint32_t lc, uint32_t rlimit) { return extract_ub(rank, lq, lc) < rlimit; }

// Whether pair (i, j) of rank r is reported.
STRSIM_HD bool join_hit(uint32_t r, uint32_t rlimit, bool upper, uint32_t i, uint32_t j) { return r < rlimit && (!upper || j > i); }

// What a pair yields in this join's sweep and what becomes of it (the rule object of join_lane_slice in strsim_join_kernels.h and of
// its host transcript, as NearestRules / ExtractRules are search_sweep_lane's): its rank, looked up in the lane's row of the rank
// table at the candidate length in hand; the f64 score is formed only for a hit that is stored.
struct JoinRankRule {
    const uint16_t *row; // rank[lq + lc]: indexed by the distance
    uint32_t rlimit;
    const uint16_t *rep;
    STRSIM_HD uint32_t value(uint32_t d) const { return row[d]; } // d <= lq + lc: inside the row
    STRSIM_HD bool hit(uint32_t r, bool upper, uint32_t i, uint32_t j) const { return join_hit(r, rlimit, upper, i, j); }
    STRSIM_HD double score(uint32_t r) const { return extract_rank_score(rep, r); }
};

// Split `split` of `splits` takes [x0, x1) of the length bucket [c0, c0 + n) of the length-ordered candidates.
STRSIM_HD void join_slice(uint32_t c0, uint32_t n, uint32_t split, uint32_t splits, uint32_t &x0, uint32_t &x1)
{
    x0 = c0 + (uint32_t)((uint64_t)n * split / splits);
    x1 = c0 + (uint32_t)((uint64_t)n * (split + 1u) / splits);
}

// Candidate splits of k_join_lane for nq queries x nc candidates.  cdist_splits' reasoning, in workgroups of 256: enough of them
// over the query workgroups to fill the device -- JOIN_WG_PER_CU = 16 per CU, two rounds of the eight that are resident, because
// the queries are in length order and a workgroup's work grows with its queries' length (a wider window of longer candidates):
// with one round the sweep takes as long as its heaviest workgroup (k_join_lane also starts the heaviest first).  At least
// JOIN_MIN_PER_SPLIT candidates per split and at most JOIN_MAX_SPLITS splits, so that the counts, (splits + 1) words per query,
// stay small: splits > 1 only while nq < 4096 * num_cu, and splits * nq is then below 256 * (16 * num_cu + nq / 256 + 1) words.
constexpr uint32_t JOIN_WG_PER_CU = 16u;
inline uint32_t join_splits(uint64_t nq, uint64_t nc, int num_cu)
{
    const uint64_t qblocks = (nq + 255u) / 256u;
    const uint64_t target = JOIN_WG_PER_CU * (uint64_t)(num_cu > 0 ? num_cu : 256);
    uint64_t s = (target + qblocks - 1u) / (qblocks ? qblocks : 1u);
    const uint64_t by_c = (nc + JOIN_MIN_PER_SPLIT - 1u) / JOIN_MIN_PER_SPLIT;
    if (s > by_c) s = by_c;
    if (s > JOIN_MAX_SPLITS) s = JOIN_MAX_SPLITS;
    return s ? (uint32_t)s : 1u;
}

// The counts of query i, cnt[l * nq + i] for its `lists` lists (the splits of the sweep, then the fallback's), into their
// exclusive prefix in place; returns their total.  List l of the query is then [indptr[i] + cnt[l * nq + i], indptr[i] +
// cnt[(l + 1) * nq + i]), the last one ends at indptr[i + 1].
STRSIM_HD uint64_t join_row_prefix(uint32_t *cnt, uint64_t nq, uint64_t i, uint32_t lists)
{
    uint64_t acc = 0;
    for (uint32_t l = 0; l < lists; ++l) {
        const uint32_t n = cnt[(uint64_t)l * nq + i];
        cnt[(uint64_t)l * nq + i] = (uint32_t)acc; // (a row has at most 2^32 - 2 hits)
        acc += n;
    }
    return acc;
}

// ---- the hit map: which candidates of a wave's sweep had a hit at all ----
// Hits are sparse (at 0.8 a few in ten thousand of the pairs the window admits), so the count sweep leaves one bit per (wave,
// group of 2^shift consecutive positions of the length order) that says whether any lane of the wave had a hit there, and the fill
// sweep computes only the candidates whose bit is set: the second sweep costs what the hits cost, not what the window costs.  A
// slice -- one (length, split) of the sweep, number k = lc * splits + split -- keeps its bits in words of its own, word
// (x >> shift >> 5) + k for position x: slices are disjoint and ordered by k, so the next slice's first word lies behind this one's
// last and every word has one writer -- plain stores, no atomics, and a fill reads only words its own count sweep wrote.  shift is
// the smallest at which the map of all waves stays within JOIN_MAP_BUDGET.
constexpr uint64_t JOIN_MAP_BUDGET = (uint64_t)256 << 20;
STRSIM_HD uint64_t join_map_words(uint64_t nc, uint32_t splits, uint32_t shift) { return (nc >> shift >> 5) + (uint64_t)NEAREST_BUCKETS * splits + 2u; }
STRSIM_HD uint32_t join_map_slice(uint32_t lc, uint32_t split, uint32_t splits) { return lc * splits + split; }
STRSIM_HD uint64_t join_map_word(uint32_t x, uint32_t shift, uint32_t k) { return (uint64_t)(x >> shift >> 5) + k; }
STRSIM_HD uint32_t join_map_bit(uint32_t x, uint32_t shift) { return 1u << ((x >> shift) & 31u); }
inline uint32_t join_map_shift(uint64_t nq, uint64_t nc, uint32_t splits)
{
    const uint64_t waves = (nq + 63u) / 64u;
    uint32_t shift = 0u;
    while (shift < 31u && waves * join_map_words(nc, splits, shift) * 4u > JOIN_MAP_BUDGET) ++shift;
    return shift;
}

// One store of the fill: (j, score) at `cur` of a segment that ends before `end`.  Nothing is written at or beyond the end.
STRSIM_HD bool join_store(uint64_t &cur, uint64_t end, uint32_t j, double score, uint32_t *out_index, double *out_score)
{
    if (cur >= end) return false;
    out_index[cur] = j;
    out_score[cur] = score;
    ++cur;
    return true;
}

// ---- the 64-bit inclusive scan of n values (the row totals, in place -> indptr[1 ..]) ----
// Workgroup b takes values [b * JOIN_SCAN_TILE, ...), thread t of it JOIN_SCAN_PER consecutive ones: [first, last).
STRSIM_HD void join_scan_range(uint64_t block, uint32_t tid, uint64_t n, uint64_t &first, uint64_t &last)
{
    first = block * JOIN_SCAN_TILE + (uint64_t)tid * JOIN_SCAN_PER;
    if (first > n) first = n;
    last = n - first < JOIN_SCAN_PER ? n : first + JOIN_SCAN_PER;
}
STRSIM_HD uint64_t join_scan_blocks(uint64_t n) { return (n + JOIN_SCAN_TILE - 1u) / JOIN_SCAN_TILE; }
STRSIM_HD uint64_t join_scan_sum(const uint64_t *v, uint64_t first, uint64_t last)
{
    uint64_t acc = 0;
    for (uint64_t x = first; x < last; ++x) acc += v[x];
    return acc;
}
// v[first .. last) into its inclusive scan on top of `base`.
STRSIM_HD void join_scan_write(uint64_t *v, uint64_t first, uint64_t last, uint64_t base)
{
    for (uint64_t x = first; x < last; ++x) { base += v[x]; v[x] = base; }
}
// The block sums of the top pass: thread t of JOIN_SCAN_BLOCK takes sums [first, last) of nb.
STRSIM_HD void join_scan_top_range(uint32_t tid, uint64_t nb, uint64_t &first, uint64_t &last)
{
    const uint64_t per = (nb + JOIN_SCAN_BLOCK - 1u) / JOIN_SCAN_BLOCK;
    first = (uint64_t)tid * per < nb ? (uint64_t)tid * per : nb;
    last = nb - first < per ? nb : first + per;
}

// ---- the row sort: the ascending-only bitonic network over the next power of two ----
// A merge stage of block size k (2, 4, .. P) is the steps of stride h = k / 2, k / 4, .. 1.  Comparator t (0 .. P / 2 - 1) of a
// step: the first step of a stage (h == k / 2) compares x with block_end - 1 - x, a later one x with x + h; a < b always and the
// smaller key goes to a.  A comparator with b >= n is skipped: the elements at and above n act as +infinity, every exchange is
// ascending, so they never move and a comparison with one never exchanges.
STRSIM_HD uint64_t join_sort_pow2(uint64_t n)
{
    uint64_t p = 1u;
    while (p < n) p <<= 1;
    return p;
}
STRSIM_HD void join_sort_pair(uint64_t t, uint64_t k, uint64_t h, uint64_t &a, uint64_t &b)
{
    const uint64_t blk = t / h, r = t - blk * h;
    a = blk * 2u * h + r;
    b = h == k / 2u ? blk * k + k - 1u - r : a + h;
}
// One comparator over a row's (index, score) pairs: the keys of a row are distinct.
STRSIM_HD void join_sort_cmpx(uint32_t *index, double *score, uint64_t a, uint64_t b)
{
    const uint32_t ia = index[a], ib = index[b];
    if (ia > ib) {
        const double sa = score[a], sb = score[b];
        index[a] = ib; index[b] = ia;
        score[a] = sb; score[b] = sa;
    }
}

} // namespace strsim
