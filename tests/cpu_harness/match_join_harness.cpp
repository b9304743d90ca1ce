// match_join_harness.cpp -- host build of the rules strsim_match_join.h shares with k_match_join_lane
// (strsim_match_join_kernels.h), for tests/test_match_join_cpu.py: g++ compiles the same headers.
//   mj_bound_check   for every pair of lengths 0 .. 32: the maximum of the measure's own epilogue over EVERY integer tuple the
//                    kernel can produce (d in |lq - lc| .. max; m <= min, t <= m, prefix <= min(4, min); isect <= min) against
//                    match_join_ub -- no tuple above the bound, and the bound attained.
//   mj_need_mask     the library's need mask of a call, for the comparison with match_join_ub >= cutoff made directly.
//   mj_replay        a wave's count sweep, the counts -> prefix -> 64-bit scan, and its fill sweep (k_match_join_lane<M, false /
//                    true>: the loop of join_harness.cpp under the new need rule, every split in turn, a ballot written as a loop over
//                    the lanes) over a random score matrix that respects the bound, against brute force: every hit found exactly once
//                    with its own score, the fill positions exactly the counted segments, a length whose bit is clear never visited,
//                    nothing written outside a segment (guard words, and one deliberately undersized segment whose last hit is
//                    refused), every word of the hit map with one writer; then the row sort.
// Built as a shared library; with -DMATCH_JOIN_HARNESS_MAIN it is a stand-alone program that runs every case (the form that is run
// under the address and undefined-behaviour sanitizers).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <numeric>
#include <vector>

#include "strsim_match_join.h"

using namespace strsim;

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

// The integers a pair's score is made of; which of them a measure reads is the measure's business.
struct Tuple {
    uint32_t d, m, t, prefix, isect;
};

// The score of a pair of lengths (lq, lc) whose cores returned `u`: the library's epilogues, the empty strings as every kernel
// answers them (1.0 for two, 0.0 for one).
static double score_of(int measure, uint32_t lq, uint32_t lc, const Tuple &u)
{
    if (lq == 0u && lc == 0u) return 1.0;
    if (lq == 0u || lc == 0u) return 0.0;
    switch (measure) {
    case LEVENSHTEIN: return epilogue_levenshtein(u.d, lq, lc);
    case JARO: return epilogue_jaro(u.m, u.t, lq, lc);
    case JARO_WINKLER: return epilogue_jaro_winkler(epilogue_jaro(u.m, u.t, lq, lc), u.prefix);
    case JACCARD: return epilogue_jaccard(u.isect, lq, lc);
    default: return epilogue_sorensen_dice(u.isect, lq, lc);
    }
}

// f(tuple) for every tuple the kernel can produce at these lengths (only the integers `measure` reads are varied).
template <class F>
static void every_tuple(int measure, uint32_t lq, uint32_t lc, F f)
{
    const uint32_t mn = std::min(lq, lc), mx = std::max(lq, lc), pmax = std::min(4u, mn);
    Tuple u{mx - mn, 0u, 0u, 0u, 0u};
    if (measure == LEVENSHTEIN) {
        for (u.d = mx - mn; u.d <= mx; ++u.d) f(u);
    } else if (measure == JARO || measure == JARO_WINKLER) {
        for (u.m = 0; u.m <= mn; ++u.m)
            for (u.t = 0; u.t <= u.m; ++u.t)
                for (u.prefix = 0; u.prefix <= (measure == JARO_WINKLER ? pmax : 0u); ++u.prefix) f(u);
    } else {
        for (u.isect = 0; u.isect <= mn; ++u.isect) f(u);
    }
}

static Tuple random_tuple(Rng &g, uint32_t lq, uint32_t lc)
{
    const uint32_t mn = std::min(lq, lc), mx = std::max(lq, lc);
    Tuple u;
    // near pairs are common: most of the time within three of the best integers
    const bool near = g.below(3) != 0u;
    u.d = near ? std::min(mx, mx - mn + g.below(4)) : mx - mn + g.below(mn + 1);
    u.m = near ? mn - g.below(std::min(mn, 3u) + 1) : g.below(mn + 1);
    u.t = near ? g.below(std::min(u.m, 2u) + 1) : g.below(u.m + 1);
    u.prefix = g.below(std::min(4u, mn) + 1);
    u.isect = near ? mn - g.below(std::min(mn, 3u) + 1) : g.below(mn + 1);
    return u;
}

extern "C" double mj_ub(int measure, uint32_t lq, uint32_t lc) { return match_join_ub(measure, lq, lc); }

// 0, or how many length pairs have a tuple above the bound or none that attains it.
extern "C" uint32_t mj_bound_check(int measure)
{
    uint32_t bad = 0;
    for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq)
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
            const double ub = match_join_ub(measure, lq, lc);
            bool above = false, attained = false;
            every_tuple(measure, lq, lc, [&](const Tuple &u) {
                const double v = score_of(measure, lq, lc, u);
                if (!(v <= ub)) above = true; // (a NaN would count too)
                if (v == ub) attained = true;
            });
            if (above || !attained) ++bad;
        }
    return bad;
}

// The library's need mask of a call into out[33]; returns whether any bit is set.
extern "C" int mj_need_mask(int measure, double cutoff, uint64_t *out)
{
    MatchJoinNeed need;
    const bool any = match_join_need_mask(measure, cutoff, need);
    memcpy(out, need.w, sizeof need.w);
    return any ? 1 : 0;
}

extern "C" uint32_t mj_lengths(void) { return MATCH_JOIN_LENGTHS; }
extern "C" uint32_t mj_need_bytes(void) { return (uint32_t)sizeof(MatchJoinNeed); }

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
    {
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

static void sort_as_kernels(uint32_t *index, double *score, uint64_t n)
{
    const uint64_t P = join_sort_pow2(n);
    for (uint64_t k = 2; k <= P; k <<= 1)
        for (uint64_t h = k >> 1; h > 0; h >>= 1)
            for (uint64_t t = P / 2; t-- > 0;) {
                uint64_t a, b;
                join_sort_pair(t, k, h, a, b);
                if (b < n) join_sort_cmpx(index, score, a, b);
            }
}

// One sweep of a wave, every split in turn: on_hit(split, i, j, v) for every pair the sweep reports (k_match_join_lane's loops).
// fill = false marks the wave's hit map, fill = true computes only the candidates marked there.  Returns the candidates computed;
// *lengths collects the lengths the wave visited.
template <class OnHit>
static uint64_t sweep(const MatchJoinNeed &need, const std::vector<uint32_t> &qlen, const std::vector<uint32_t> &order, const uint32_t *cstart,
                      const double *score, uint32_t nc, double cutoff, bool upper, uint32_t splits, bool fill, uint32_t shift,
                      std::vector<uint32_t> &map, std::vector<uint8_t> &map_writes, uint64_t *lengths, OnHit on_hit)
{
    const uint32_t nq = (uint32_t)qlen.size();
    uint64_t visited = 0;
    // the lane's word and the wave's: the kernel's loop over the 33 words with a uniform index
    std::vector<uint64_t> mine(nq, 0);
    uint64_t wave = 0;
    for (uint32_t l = 0; l < MATCH_JOIN_LENGTHS; ++l) {
        const uint64_t w = need.w[l];
        bool any = false;
        for (uint32_t i = 0; i < nq; ++i)
            if (qlen[i] == l) { mine[i] = w; any = true; }
        if (any) wave |= w;
    }
    auto flush = [&](uint64_t at, uint32_t bits) { // one writer per word, and inside the wave's map
        if (fill || at == ~0ull) return;
        map.at(at) = bits;
        ++map_writes.at(at);
    };
    for (uint32_t split = 0; split < splits; ++split)
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
            if (!((wave >> lc) & 1ull)) continue;
            *lengths |= 1ull << lc;
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
                    const double v = score[(size_t)i * nc + j];
                    const bool nd = ((mine[i] >> lc) & 1ull) != 0ull;
                    if (nd && match_join_hit(v, cutoff, upper, i, j)) { on_hit(split, i, j, v); any_hit = true; }
                }
                if (!fill && any_hit) bits |= bit;
            }
            flush(at, bits);
        }
    return visited;
}

// nq <= 64 queries and nc candidates of random lengths 0 .. maxlen, every pair's score the measure's epilogue of a random tuple;
// stats[0] = candidates visited by one sweep (out of nc), stats[1] = hits, stats[2] = the lengths the count sweep visited (bits).
// 0, or the number of the first check that failed.
extern "C" int mj_replay(uint64_t seed, int measure, uint32_t nq, uint32_t nc, uint32_t maxlen, double cutoff, int upper, uint32_t splits,
                         int undersize, uint32_t shift, uint64_t *stats)
{
    Rng g{seed * 2654435761ull + 12345u + (uint64_t)measure * 977u};
    std::vector<uint32_t> qlen(nq), clen(nc);
    std::vector<double> score((size_t)nq * nc);
    for (auto &l : qlen) l = g.below(maxlen + 1);
    for (auto &l : clen) l = g.below(maxlen + 1);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < nc; ++j) score[(size_t)i * nc + j] = score_of(measure, qlen[i], clen[j], random_tuple(g, qlen[i], clen[j]));
    stats[0] = stats[1] = stats[2] = 0;
    // brute force
    std::vector<std::vector<uint32_t>> want(nq);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < nc; ++j)
            if (score[(size_t)i * nc + j] >= cutoff && (!upper || j > i)) want[i].push_back(j);
    MatchJoinNeed need;
    if (!match_join_need_mask(measure, cutoff, need) || nq == 0u) { // (the library launches no sweep)
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
    // the lengths some query needs: the union the sweep may visit and nothing else
    uint64_t allowed = 0;
    for (uint32_t i = 0; i < nq; ++i) allowed |= need.w[qlen[i]];

    // count
    const uint32_t lists = splits + 1;
    std::vector<uint32_t> cnt((size_t)lists * nq, 0);
    std::vector<uint32_t> map(join_map_words(nc, splits, shift), 0xA5A5A5A5u);
    std::vector<uint8_t> map_writes(map.size(), 0);
    uint64_t seen = 0;
    stats[0] = sweep(need, qlen, order, cstart, score.data(), nc, cutoff, upper != 0, splits, false, shift, map, map_writes, &seen,
                     [&](uint32_t s, uint32_t i, uint32_t, double) { ++cnt[(size_t)s * nq + i]; });
    stats[2] = seen;
    if (seen != allowed) return 13; // exactly the lengths whose bit is set in some live lane's word
    for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) // (and a clear bit is a true statement: no hit was lost to it)
        for (uint32_t i = 0; i < nq; ++i)
            if (!match_join_needs(need, qlen[i], lc) && match_join_ub(measure, qlen[i], lc) >= cutoff) return 14;
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
    uint64_t seen_fill = 0;
    const uint64_t again = sweep(need, qlen, order, cstart, score.data(), nc, cutoff, upper != 0, splits, true, shift, map, map_writes, &seen_fill,
                                 [&](uint32_t s, uint32_t i, uint32_t j, double v) {
                                     uint64_t &c = cur[(size_t)s * nq + i];
                                     const uint64_t at = c;
                                     if (join_store(c, end[(size_t)s * nq + i], j, v, out_index, out_score)) {
                                         if (at < indptr[i] || at >= indptr[i + 1]) bad = 4;
                                         if (++writes[EDGE + at] > 1) bad = 5;
                                     } else ++refused;
                                 });
    if (bad) return bad;
    if (seen_fill != allowed) return 13;
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
            if (memcmp(&score[(size_t)i * nc + j], &out_score[r0 + x], 8)) return 10;
        }
    }
    for (size_t x = 0; x < EDGE; ++x)
        if (oi[x] != GUARD_I || oi[EDGE + nnz + x] != GUARD_I || !is_guard(os[x]) || !is_guard(os[EDGE + nnz + x])) return 11;
    return 0;
}

// The cutoffs of the suite for a measure: -inf, 0, 0.5, 0.8, 1.0, 1.5, and ub(measure, 7, 9) with its two f64 neighbours.
extern "C" uint32_t mj_cutoffs(int measure, double *out)
{
    const double e = match_join_ub(measure, 7, 9), inf = std::numeric_limits<double>::infinity();
    const double cuts[9] = {-inf, 0.0, 0.5, 0.8, 1.0, 1.5, nextafter(e, 0.0), e, nextafter(e, 2.0)};
    memcpy(out, cuts, sizeof cuts);
    return 9u;
}

// Every case of the sweep; the count of failures.
extern "C" uint32_t mj_replay_all(void)
{
    uint32_t failed = 0;
    uint64_t stats[3];
    double cuts[9];
    for (int measure = 0; measure < 5; ++measure) {
        const uint32_t ncuts = mj_cutoffs(measure, cuts);
        for (uint32_t c = 0; c < ncuts; ++c)
            for (int upper = 0; upper < 2; ++upper)
                for (uint32_t splits = 1; splits <= 3; ++splits)
                    for (uint32_t shift = 0; shift < 3; ++shift) // hit-map groups of 1, 2 and 4 positions
                        for (int under = 0; under < 2; ++under)
                            for (uint64_t seed = 0; seed < 4; ++seed) {
                                const uint32_t nq = seed == 0 ? 1u : seed == 1 ? 64u : 1u + (uint32_t)(seed * 11u);
                                const uint32_t nc = seed == 2 ? 0u : 40u + (uint32_t)seed * 37u;
                                if (mj_replay(seed + 100 * c, measure, nq, nc, seed == 3 ? 6u : 32u, cuts[c], upper, splits, under, shift, stats)) ++failed;
                            }
    }
    return failed;
}

#ifdef MATCH_JOIN_HARNESS_MAIN
int main()
{
    uint32_t bounds = 0, masks = 0;
    double cuts[9];
    for (int measure = 0; measure < 5; ++measure) {
        bounds += mj_bound_check(measure);
        const uint32_t ncuts = mj_cutoffs(measure, cuts);
        for (uint32_t c = 0; c < ncuts; ++c) {
            uint64_t w[MATCH_JOIN_LENGTHS];
            mj_need_mask(measure, cuts[c], w);
            for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq)
                for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc)
                    masks += (((w[lq] >> lc) & 1ull) != 0ull) != (match_join_ub(measure, lq, lc) >= cuts[c]);
        }
    }
    const uint32_t failed = mj_replay_all();
    printf("match_join harness: %u length pairs off their bound, %u mask bits differ, %u replays failed\n", bounds, masks, failed);
    return bounds || masks || failed ? 1 : 0;
}
#endif
