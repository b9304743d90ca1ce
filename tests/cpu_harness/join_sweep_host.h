// The sweep of one wave of the join kernels (join_lane_slice of strsim_join_kernels.h, under k_join_lane<FILL> and
// k_match_join_lane<M, FILL>) on the host, and the replay of the protocol around it: the same statements under the rule objects the
// kernels run (JoinRankRule of strsim_join.h, MatchJoinRule of strsim_match_join.h), with a ballot written as a loop over the lanes.
// Shared by join_harness.cpp and match_join_harness.cpp, which bring what differs: the loop over the candidate lengths, what a pair
// yields and the score it must end with.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "strsim_join.h"

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0u; }
};

static const uint32_t GUARD_I = 0xDEADBEEFu;
static const uint64_t GUARD_S = 0x7FF8DEADBEEF0001ull; // a NaN payload no score has
static const size_t EDGE = 8;

inline double guard_score() { double g; memcpy(&g, &GUARD_S, 8); return g; }
inline bool is_guard(double v) { uint64_t b; memcpy(&b, &v, 8); return b == GUARD_S; }

// The 64-bit inclusive scan of v[0 .. n) as k_join_scan_sums / _top / _apply partition it.
inline void scan_as_kernels(std::vector<uint64_t> &v)
{
    using namespace strsim;
    const uint64_t n = v.size(), nb = join_scan_blocks(n);
    std::vector<uint64_t> sums(nb ? nb : 1, 0);
    for (uint64_t b = 0; b < nb; ++b)
        for (uint32_t t = 0; t < JOIN_SCAN_BLOCK; ++t) {
            uint64_t first, last;
            join_scan_range(b, t, n, first, last);
            sums[b] += join_scan_sum(v.data(), first, last);
        }
    { // the top pass: thread t's base is the sum of the chunks of the threads before it
        uint64_t base = 0;
        for (uint32_t t = 0; t < JOIN_SCAN_BLOCK; ++t) {
            uint64_t first, last;
            join_scan_top_range(t, nb, first, last);
            for (uint64_t x = first; x < last; ++x) { const uint64_t s = sums[x]; sums[x] = base; base += s; }
        }
    }
    for (uint64_t b = 0; b < nb; ++b) {
        uint64_t base = 0;
        for (uint32_t t = 0; t < JOIN_SCAN_BLOCK; ++t) {
            uint64_t first, last;
            join_scan_range(b, t, n, first, last);
            const uint64_t mine = join_scan_sum(v.data(), first, last);
            join_scan_write(v.data(), first, last, sums[b] + base);
            base += mine;
        }
    }
}

// The network of k_join_sort_rows over a row of n pairs: every comparator of every step, in any order inside a step.
inline void sort_as_kernels(uint32_t *index, double *score, uint64_t n)
{
    using namespace strsim;
    const uint64_t P = join_sort_pow2(n);
    for (uint64_t k = 2; k <= P; k <<= 1)
        for (uint64_t h = k >> 1; h > 0; h >>= 1)
            for (uint64_t t = P / 2; t-- > 0;) { // (descending: the order inside a step must not matter)
                uint64_t a, b;
                join_sort_pair(t, k, h, a, b);
                if (b < n) join_sort_cmpx(index, score, a, b);
            }
}

// A wave of nq <= 64 lanes between its two sweeps: the kernels' arguments (JoinSweep) and, for every (split, lane), what a lane
// keeps in registers -- its count, or its cursor and its segment's end -- with the replay's own bookkeeping beside them.
struct JoinWave {
    uint32_t nq, nc, splits, shift;
    bool upper;
    std::vector<uint32_t> order;                  // the candidates in length order
    uint32_t cstart[strsim::NEAREST_BUCKETS + 1]; // the length buckets of that order
    std::vector<uint32_t> map;                    // the wave's hit map
    std::vector<uint8_t> map_writes;              // stores into each of its words
    std::vector<uint32_t> cnt;                    // (splits + 1) x nq: the counts, then their prefix
    std::vector<uint64_t> indptr, cur, end;       // cur, end: [split * nq + i], the fill's segments
    uint32_t *out_index;
    double *out_score;
    std::vector<uint8_t> writes; // stores into each output position (EDGE guard words in front)
    uint64_t visited;            // candidates computed by the sweep in hand
    uint32_t refused;            // stores join_store turned down
    int bad;                     // check 4 or 5, if one failed
};

// join_lane_slice for every lane of the wave: the candidates of length lc that `split` takes.  need(i): lane i's own need of this
// length; rule(i): its rule object at this length; core(i, j): what the kernel's scoring call returns for the pair (a distance, a
// score).  fill = false counts and marks the hit map, fill = true computes only the candidates marked there and stores into the lanes' segments.
template <class Need, class RuleAt, class Core>
void join_slice_host(JoinWave &W, bool fill, uint32_t split, uint32_t lc, Need need, RuleAt rule, Core core)
{
    using namespace strsim;
    auto flush = [&](uint64_t at, uint32_t bits) { // one writer per word, and inside the wave's map
        if (fill || at == ~0ull) return;
        W.map.at(at) = bits;
        ++W.map_writes.at(at);
    };
    uint32_t x0, x1;
    join_slice(W.cstart[lc], W.cstart[lc + 1] - W.cstart[lc], split, W.splits, x0, x1);
    const uint32_t k = join_map_slice(lc, split, W.splits);
    uint64_t at = ~0ull; // the word of the hit map in hand, its bits
    uint32_t bits = 0;
    for (uint32_t x = x0; x < x1; ++x) {
        const uint64_t w = join_map_word(x, W.shift, k);
        if (w != at) {
            flush(at, bits);
            at = w;
            bits = fill ? W.map.at(w) : 0u;
        }
        const uint32_t bit = join_map_bit(x, W.shift);
        if (fill && !(bits & bit)) continue; // no lane of the wave had a hit in this group
        const uint32_t j = W.order[x];
        ++W.visited;
        bool any_hit = false; // the ballot
        for (uint32_t i = 0; i < W.nq; ++i) {
            const auto R = rule(i);
            const auto v = R.value(core(i, j));
            if (!(need(i) && R.hit(v, W.upper, i, j))) continue;
            any_hit = true;
            const size_t l = (size_t)split * W.nq + i;
            if (!fill) { ++W.cnt[l]; continue; }
            const uint64_t to = W.cur[l];
            if (join_store(W.cur[l], W.end[l], j, R.score(v), W.out_index, W.out_score)) {
                if (to < W.indptr[i] || to >= W.indptr[i + 1]) W.bad = 4;
                if (++W.writes[EDGE + to] > 1) W.bad = 5;
            } else ++W.refused;
        }
        if (!fill && any_hit) bits |= bit;
    }
    flush(at, bits);
}

// The protocol of a join over one wave: nq <= 64 queries against nc candidates of lengths clen.  A count sweep, the counts ->
// prefix -> 64-bit scan, and a fill sweep, every split in turn, against brute force: every hit found exactly once with its own
// score, the fill positions exactly the counted segments, nothing written outside a segment (guard words around the outputs, and
// with `undersize` one segment that is one slot short), every word of the hit map with one writer, the fill computing the marked
// candidates only; then the row sort.  What a Case brings:
//   nothing                  the library launches no sweep: no pair may be a hit
//   cutoff, expected(i, j)   the score pair (i, j) must end with; it is a hit iff expected >= cutoff (and j > i under upper)
//   lengths(W, fill, split)  a split's loop over the candidate lengths as its kernel makes it: join_slice_host for every length visited
//   after(W, fill)           checks of its own after a sweep (0: none failed)
// stats[0] = candidates computed by the count sweep (out of nc per split), stats[1] = hits.  0, or the number of the first check
// that failed.
template <class Case>
int join_replay_host(Case &C, uint32_t nq, const std::vector<uint32_t> &clen, bool upper, uint32_t splits, int undersize, uint32_t shift,
                     uint64_t *stats)
{
    using namespace strsim;
    const uint32_t nc = (uint32_t)clen.size();
    stats[0] = stats[1] = 0;
    // brute force
    std::vector<std::vector<uint32_t>> want(nq);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < nc; ++j)
            if (C.expected(i, j) >= C.cutoff && (!upper || j > i)) want[i].push_back(j);
    if (C.nothing || nq == 0u) {
        for (auto &w : want) if (!w.empty()) return 1;
        return 0;
    }
    JoinWave W{};
    W.nq = nq, W.nc = nc, W.splits = splits, W.shift = shift, W.upper = upper;
    // the length order: any order inside a length (here, descending index)
    W.order.resize(nc);
    std::iota(W.order.begin(), W.order.end(), 0u);
    std::stable_sort(W.order.begin(), W.order.end(), [&](uint32_t a, uint32_t b) { return clen[a] != clen[b] ? clen[a] < clen[b] : a > b; });
    for (uint32_t j = 0; j < nc; ++j) ++W.cstart[clen[j] + 1];
    for (uint32_t b = 0; b < NEAREST_BUCKETS; ++b) W.cstart[b + 1] += W.cstart[b];

    // count
    const uint32_t lists = splits + 1;
    W.cnt.assign((size_t)lists * nq, 0);
    W.map.assign(join_map_words(nc, splits, shift), 0xA5A5A5A5u);
    W.map_writes.assign(W.map.size(), 0);
    for (uint32_t split = 0; split < splits; ++split) C.lengths(W, false, split);
    stats[0] = W.visited;
    if (const int r = C.after(W, false)) return r;
    const std::vector<uint32_t> raw = W.cnt;
    std::vector<uint64_t> tot(nq);
    W.indptr.assign(nq + 1, 0);
    for (uint32_t i = 0; i < nq; ++i) tot[i] = join_row_prefix(W.cnt.data(), nq, i, lists);
    scan_as_kernels(tot);
    for (uint32_t i = 0; i < nq; ++i) W.indptr[i + 1] = tot[i];
    const std::vector<uint64_t> &indptr = W.indptr;
    const uint64_t nnz = indptr[nq];
    stats[1] = nnz;
    for (uint32_t i = 0; i < nq; ++i)
        if (indptr[i + 1] - indptr[i] != want[i].size()) return 2;

    // fill, guard words around the outputs
    std::vector<uint32_t> oi(nnz + 2 * EDGE, GUARD_I);
    std::vector<double> os(nnz + 2 * EDGE, guard_score());
    W.writes.assign(nnz + 2 * EDGE, 0);
    W.out_index = oi.data() + EDGE;
    W.out_score = os.data() + EDGE;
    W.cur.resize((size_t)splits * nq), W.end.resize((size_t)splits * nq);
    int64_t short_at = -1; // the undersized segment: its last slot is taken away
    for (uint32_t s = 0; s < splits; ++s)
        for (uint32_t i = 0; i < nq; ++i) {
            const size_t l = (size_t)s * nq + i;
            W.cur[l] = indptr[i] + W.cnt[l];
            W.end[l] = indptr[i] + W.cnt[l + nq];
            if (W.end[l] - W.cur[l] != raw[l]) return 3;
            if (undersize && short_at < 0 && raw[l]) { short_at = (int64_t)--W.end[l]; }
        }
    for (uint8_t n : W.map_writes)
        if (n > 1) return 12; // every word of the hit map has one writer
    W.visited = 0;
    for (uint32_t split = 0; split < splits; ++split) C.lengths(W, true, split);
    if (W.bad) return W.bad;
    if (const int r = C.after(W, true)) return r;
    if (W.visited > stats[0] || W.visited > (nnz << shift)) return 6; // the fill computes marked candidates only: at most 2^shift per hit
    if (W.refused != (short_at >= 0 ? 1u : 0u)) return 7;
    for (size_t x = 0; x < oi.size(); ++x) {
        const bool inside = x >= EDGE && x < EDGE + nnz && (int64_t)(x - EDGE) != short_at;
        if (inside ? W.writes[x] != 1 : (W.writes[x] || oi[x] != GUARD_I || !is_guard(os[x]))) return 8;
    }
    if (short_at >= 0) return 0; // (the row with the hole is not a result)
    // every hit exactly once, with its own score; then the row sort
    for (uint32_t i = 0; i < nq; ++i) {
        const uint64_t r0 = indptr[i], n = indptr[i + 1] - r0;
        sort_as_kernels(W.out_index + r0, W.out_score + r0, n);
        for (uint64_t x = 0; x < n; ++x) {
            const uint32_t j = W.out_index[r0 + x];
            if (j != want[i][x]) return 9;
            const double e = C.expected(i, j);
            if (memcmp(&e, &W.out_score[r0 + x], 8)) return 10;
        }
    }
    for (size_t x = 0; x < EDGE; ++x)
        if (oi[x] != GUARD_I || oi[EDGE + nnz + x] != GUARD_I || !is_guard(os[x]) || !is_guard(os[EDGE + nnz + x])) return 11;
    return 0;
}
