// join_harness.cpp -- host build of the rules strsim_join.h shares with the join kernels (strsim_join_kernels.h), for
// tests/test_join_cpu.py: g++ compiles the same header.
//   join_replay      a wave's count sweep, the counts -> prefix -> 64-bit scan, and its fill sweep (k_join_lane<false / true>, every
//                    split in turn, a ballot written as a loop over the lanes) over a random (d, s) matrix against brute force:
//                    every hit found exactly once with its own score, the fill positions exactly the counted segments, nothing
//                    written outside a segment (guard words around the outputs, and one deliberately undersized segment), then the
//                    row sort; the count sweep marks the hit map and the fill sweep computes the marked candidates only (every word of
//                    the map has one writer); reports how many candidates the count sweep visited.
//   join_sort_check  the comparator network of k_join_sort_rows over n distinct keys against std::sort, guard words around the row.
//   join_scan_check  the three passes of the 64-bit scan as the kernels partition them, against a serial prefix sum.
// Built as a shared library; with -DJOIN_HARNESS_MAIN it is a stand-alone program that runs the whole sweep of cases (the form
// that is run under the address and undefined-behaviour sanitizers).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <numeric>
#include <vector>

#include "strsim_join.h"

using namespace strsim;

static const ExtractTable &table()
{
    static const ExtractTable *const t = [] {
        ExtractTable *n = new ExtractTable;
        extract_build_table(*n);
        return n;
    }();
    return *t;
}

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0u; }
};

static const uint32_t GUARD_I = 0xDEADBEEFu;
static const uint64_t GUARD_S = 0x7FF8DEADBEEF0001ull; // a NaN payload no score has
static const size_t EDGE = 8;

static double guard_score() { double g; memcpy(&g, &GUARD_S, 8); return g; }
static bool is_guard(double v) { uint64_t b; memcpy(&b, &v, 8); return b == GUARD_S; }

// The 64-bit inclusive scan of v[0 .. n) as k_join_scan_sums / _top / _apply partition it.
static void scan_as_kernels(std::vector<uint64_t> &v)
{
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
static void sort_as_kernels(uint32_t *index, double *score, uint64_t n)
{
    const uint64_t P = join_sort_pow2(n);
    for (uint64_t k = 2; k <= P; k <<= 1)
        for (uint64_t h = k >> 1; h > 0; h >>= 1)
            for (uint64_t t = P / 2; t-- > 0;) { // (descending: the order inside a step must not matter)
                uint64_t a, b;
                join_sort_pair(t, k, h, a, b);
                if (b < n) join_sort_cmpx(index, score, a, b);
            }
}

// One sweep of a wave, every split in turn: on_hit(split, i, j, r) for every pair the sweep reports.  fill = false marks the
// wave's hit map, fill = true computes only the candidates marked there (k_join_lane's candidate loop).  Returns the candidates
// computed.
template <class OnHit>
static uint64_t sweep(const std::vector<uint32_t> &qlen, const std::vector<uint32_t> &order, const uint32_t *cstart, const uint32_t *dist,
                      uint32_t nc, uint32_t rlimit, bool upper, uint32_t splits, bool fill, uint32_t shift, std::vector<uint32_t> &map,
                      std::vector<uint8_t> &map_writes, OnHit on_hit)
{
    const uint16_t *const rank = table().rank;
    const uint32_t nq = (uint32_t)qlen.size();
    uint64_t visited = 0;
    uint32_t lmin = 0xFFFFFFFFu, lmax = 0u;
    for (uint32_t i = 0; i < nq; ++i) { lmin = std::min(lmin, qlen[i]); lmax = std::max(lmax, qlen[i]); }
    auto flush = [&](uint64_t at, uint32_t bits) { // one writer per word, and inside the wave's map
        if (fill || at == ~0ull) return;
        map.at(at) = bits;
        ++map_writes.at(at);
    };
    for (uint32_t split = 0; split < splits; ++split) {
        uint32_t lo, hi;
        extract_window(rank, lmin, lmax, rlimit, lo, hi);
        const uint32_t steps = nearest_steps(lmin, lmax, lo, hi);
        for (uint32_t g = 0; g < steps; ++g) {
            uint32_t first, last, stride;
            if (!nearest_step_range(lmin, lmax, lo, hi, g, first, last, stride)) continue;
            bool needed = false;
            for (uint32_t lc = first; lc <= last; lc += stride) {
                std::vector<uint8_t> need(nq);
                bool any = false;
                for (uint32_t i = 0; i < nq; ++i) any |= (need[i] = join_needs(rank, qlen[i], lc, rlimit));
                if (!any) continue;
                needed = true;
                uint32_t x0, x1;
                join_slice(cstart[lc], cstart[lc + 1] - cstart[lc], split, splits, x0, x1);
                const uint32_t k = join_map_slice(lc, split, splits);
                uint64_t at = ~0ull;
                uint32_t bits = 0;
                for (uint32_t x = x0; x < x1; ++x) {
                    const uint64_t w = join_map_word(x, shift, k);
                    if (w != at) {
                        flush(at, bits);
                        at = w;
                        bits = fill ? map.at(w) : 0u;
                    }
                    const uint32_t bit = join_map_bit(x, shift);
                    if (fill && !(bits & bit)) continue;
                    const uint32_t j = order[x];
                    ++visited;
                    bool any_hit = false;
                    for (uint32_t i = 0; i < nq; ++i) {
                        const uint32_t r = extract_rank(rank, dist[(size_t)i * nc + j], qlen[i] + lc);
                        if (need[i] && join_hit(r, rlimit, upper, i, j)) { on_hit(split, i, j, r); any_hit = true; }
                    }
                    if (!fill && any_hit) bits |= bit;
                }
                flush(at, bits);
            }
            if (!needed) break;
        }
    }
    return visited;
}

// nq <= 64 queries and nc candidates of random lengths 0 .. maxlen with random Indel distances; stats[0] = candidates visited by
// one sweep (out of nc), stats[1] = hits.  0, or the number of the first check that failed.
extern "C" int join_replay(uint64_t seed, uint32_t nq, uint32_t nc, uint32_t maxlen, double cutoff, int upper, uint32_t splits, int undersize,
                           uint64_t *stats)
{
    Rng g{seed * 2654435761ull + 12345u};
    std::vector<uint32_t> qlen(nq), clen(nc), dist((size_t)nq * nc);
    for (auto &l : qlen) l = g.below(maxlen + 1);
    for (auto &l : clen) l = g.below(maxlen + 1);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < nc; ++j) { // d = lq + lc - 2 lcs, lcs in 0 .. min(lq, lc); short distances are common
            const uint32_t m = std::min(qlen[i], clen[j]);
            const uint32_t lcs = g.below(3) ? m - g.below(std::min(m, 3u) + 1) : g.below(m + 1);
            dist[(size_t)i * nc + j] = qlen[i] + clen[j] - 2 * lcs;
        }
    const uint32_t rlimit = extract_rank_limit(table(), cutoff);
    stats[0] = stats[1] = 0;
    // brute force
    std::vector<std::vector<uint32_t>> want(nq);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < nc; ++j)
            if (epilogue_indel(dist[(size_t)i * nc + j], qlen[i] + clen[j], 0u) >= cutoff && (!upper || j > i)) want[i].push_back(j);
    if (rlimit == 0u || nq == 0u) { // (the library launches no sweep)
        for (auto &w : want) if (!w.empty()) return 1;
        return 0;
    }
    // the length order: any order inside a length (here, descending index)
    std::vector<uint32_t> order(nc);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return clen[a] != clen[b] ? clen[a] < clen[b] : a > b; });
    uint32_t cstart[NEAREST_BUCKETS + 1] = {};
    for (uint32_t j = 0; j < nc; ++j) ++cstart[clen[j] + 1];
    for (uint32_t b = 0; b < NEAREST_BUCKETS; ++b) cstart[b + 1] += cstart[b];

    // count
    const uint32_t lists = splits + 1;
    std::vector<uint32_t> cnt((size_t)lists * nq, 0);
    const uint32_t shift = (uint32_t)(seed % 3u); // groups of 1, 2 and 4 positions
    std::vector<uint32_t> map(join_map_words(nc, splits, shift), 0xA5A5A5A5u);
    std::vector<uint8_t> map_writes(map.size(), 0);
    stats[0] = sweep(qlen, order, cstart, dist.data(), nc, rlimit, upper != 0, splits, false, shift, map, map_writes, [&](uint32_t s, uint32_t i, uint32_t, uint32_t) { ++cnt[(size_t)s * nq + i]; });
    const std::vector<uint32_t> raw = cnt;
    std::vector<uint64_t> indptr(nq + 1, 0), tot(nq);
    for (uint32_t i = 0; i < nq; ++i) tot[i] = join_row_prefix(cnt.data(), nq, i, lists);
    scan_as_kernels(tot);
    for (uint32_t i = 0; i < nq; ++i) indptr[i + 1] = tot[i];
    const uint64_t nnz = indptr[nq];
    stats[1] = nnz;
    for (uint32_t i = 0; i < nq; ++i)
        if (indptr[i + 1] - indptr[i] != want[i].size()) return 2;

    // fill, guard words around the outputs
    std::vector<uint32_t> oi(nnz + 2 * EDGE, GUARD_I);
    std::vector<double> os(nnz + 2 * EDGE, guard_score());
    std::vector<uint8_t> writes(nnz + 2 * EDGE, 0);
    uint32_t *const out_index = oi.data() + EDGE;
    double *const out_score = os.data() + EDGE;
    std::vector<uint64_t> cur((size_t)splits * nq), end((size_t)splits * nq);
    int64_t short_at = -1; // the undersized segment: its last slot is taken away
    for (uint32_t s = 0; s < splits; ++s)
        for (uint32_t i = 0; i < nq; ++i) {
            cur[(size_t)s * nq + i] = indptr[i] + cnt[(size_t)s * nq + i];
            end[(size_t)s * nq + i] = indptr[i] + cnt[(size_t)(s + 1) * nq + i];
            if (end[(size_t)s * nq + i] - cur[(size_t)s * nq + i] != raw[(size_t)s * nq + i]) return 3;
            if (undersize && short_at < 0 && raw[(size_t)s * nq + i]) { short_at = (int64_t)--end[(size_t)s * nq + i]; }
        }
    int bad = 0;
    uint32_t refused = 0;
    for (uint8_t n : map_writes)
        if (n > 1) return 12; // every word of the hit map has one writer
    const uint64_t again = sweep(qlen, order, cstart, dist.data(), nc, rlimit, upper != 0, splits, true, shift, map, map_writes, [&](uint32_t s, uint32_t i, uint32_t j, uint32_t r) {
        uint64_t &c = cur[(size_t)s * nq + i];
        const uint64_t at = c;
        if (join_store(c, end[(size_t)s * nq + i], j, extract_rank_score(table().rep, r), out_index, out_score)) {
            if (at < indptr[i] || at >= indptr[i + 1]) bad = 4;
            if (++writes[EDGE + at] > 1) bad = 5;
        } else ++refused;
    });
    if (bad) return bad;
    if (again > stats[0] || again > (nnz << shift)) return 6; // the fill computes marked candidates only: at most 2^shift per hit
    if (refused != (short_at >= 0 ? 1u : 0u)) return 7;
    for (size_t x = 0; x < oi.size(); ++x) {
        const bool inside = x >= EDGE && x < EDGE + nnz && (int64_t)(x - EDGE) != short_at;
        if (inside ? writes[x] != 1 : (writes[x] || oi[x] != GUARD_I || !is_guard(os[x]))) return 8;
    }
    if (short_at >= 0) return 0; // (the row with the hole is not a result)
    // every hit exactly once, with its own score; then the row sort
    for (uint32_t i = 0; i < nq; ++i) {
        const uint64_t r0 = indptr[i], n = indptr[i + 1] - r0;
        sort_as_kernels(out_index + r0, out_score + r0, n);
        for (uint64_t x = 0; x < n; ++x) {
            const uint32_t j = out_index[r0 + x];
            if (j != want[i][x]) return 9;
            const double e = epilogue_indel(dist[(size_t)i * nc + j], qlen[i] + clen[j], 0u);
            if (memcmp(&e, &out_score[r0 + x], 8)) return 10;
        }
    }
    for (size_t x = 0; x < EDGE; ++x)
        if (oi[x] != GUARD_I || oi[EDGE + nnz + x] != GUARD_I || !is_guard(os[x]) || !is_guard(os[EDGE + nnz + x])) return 11;
    return 0;
}

// A row of n distinct keys in random order, each with a score of its own, guard words around it.
extern "C" int join_sort_check(uint64_t n, uint64_t seed)
{
    Rng g{seed + n * 977u};
    std::vector<uint32_t> keys(n);
    for (uint64_t x = 0; x < n; ++x) keys[x] = (uint32_t)(3 * x + 1);
    for (uint64_t x = n; x > 1; --x) std::swap(keys[x - 1], keys[g.below((uint32_t)x)]);
    std::vector<uint32_t> oi(n + 2 * EDGE, GUARD_I);
    std::vector<double> os(n + 2 * EDGE, guard_score());
    for (uint64_t x = 0; x < n; ++x) { oi[EDGE + x] = keys[x]; os[EDGE + x] = (double)keys[x] * 0.5; }
    sort_as_kernels(oi.data() + EDGE, os.data() + EDGE, n);
    std::sort(keys.begin(), keys.end());
    for (uint64_t x = 0; x < n; ++x)
        if (oi[EDGE + x] != keys[x] || os[EDGE + x] != (double)keys[x] * 0.5) return 1;
    for (size_t x = 0; x < EDGE; ++x)
        if (oi[x] != GUARD_I || oi[EDGE + n + x] != GUARD_I || !is_guard(os[x]) || !is_guard(os[EDGE + n + x])) return 2;
    return 0;
}

// n values of `each` (+ their position's low bits): the scan as the kernels partition it against a serial one; *total = the last.
extern "C" int join_scan_check(uint64_t n, uint64_t each, uint64_t *total)
{
    std::vector<uint64_t> v(n), want(n);
    uint64_t acc = 0;
    for (uint64_t x = 0; x < n; ++x) { v[x] = each + (x & 7u); acc += v[x]; want[x] = acc; }
    scan_as_kernels(v);
    *total = n ? v[n - 1] : 0;
    return v == want ? 0 : 1;
}

extern "C" uint32_t join_splits_h(uint64_t nq, uint64_t nc, int num_cu) { return join_splits(nq, nc, num_cu); }
extern "C" uint32_t join_sort_wave_max(void) { return JOIN_SORT_WAVE_MAX; }
extern "C" uint32_t join_max_splits(void) { return JOIN_MAX_SPLITS; }
extern "C" uint32_t join_min_per_split(void) { return JOIN_MIN_PER_SPLIT; }
extern "C" uint32_t join_wg_per_cu(void) { return JOIN_WG_PER_CU; }
extern "C" uint32_t join_map_shift_h(uint64_t nq, uint64_t nc, uint32_t splits) { return join_map_shift(nq, nc, splits); }
extern "C" uint64_t join_map_words_h(uint64_t nc, uint32_t splits, uint32_t shift) { return join_map_words(nc, splits, shift); }
extern "C" double join_pair_score(uint32_t d, uint32_t s) { return epilogue_indel(d, s, 0u); }

// Every case of the sweep; the count of failures.
extern "C" uint32_t join_replay_all(void)
{
    const double e = epilogue_indel(2, 6, 0u), inf = std::numeric_limits<double>::infinity();
    const double cuts[8] = {-inf, 0.0, 0.5, nextafter(e, 0.0), e, nextafter(e, 2.0), 1.0, 1.5};
    uint32_t failed = 0;
    uint64_t stats[2];
    for (uint32_t c = 0; c < 8; ++c)
        for (int upper = 0; upper < 2; ++upper)
            for (uint32_t splits = 1; splits <= 3; ++splits)
                for (int under = 0; under < 2; ++under)
                    for (uint64_t seed = 0; seed < 6; ++seed) {
                        const uint32_t nq = seed == 0 ? 1u : seed == 1 ? 64u : 1u + (uint32_t)(seed * 11u);
                        const uint32_t nc = seed == 2 ? 0u : 40u + (uint32_t)seed * 37u;
                        if (join_replay(seed + 100 * c, nq, nc, seed == 3 ? 6u : 32u, cuts[c], upper, splits, under, stats)) ++failed;
                    }
    return failed;
}

#ifdef JOIN_HARNESS_MAIN
int main()
{
    const uint32_t failed = join_replay_all();
    uint32_t sort_bad = 0, scan_bad = 0;
    for (uint64_t n = 0; n <= 130; ++n) sort_bad += join_sort_check(n, 1) != 0;
    for (uint64_t n : {510ull, 511ull, 512ull, 513ull, 1000ull, 4097ull}) sort_bad += join_sort_check(n, 2) != 0;
    uint64_t total = 0;
    for (uint64_t n : {0ull, 1ull, 7ull, 2047ull, 2048ull, 2049ull, 100000ull}) scan_bad += join_scan_check(n, 1ull << 31, &total) != 0;
    const bool wide = total > (1ull << 32);
    printf("join harness: %u replays failed, %u sorts differ, %u scans differ, totals %s 2^32\n", failed, sort_bad, scan_bad, wide ? "beyond" : "WITHIN");
    return failed || sort_bad || scan_bad || !wide ? 1 : 0;
}
#endif
