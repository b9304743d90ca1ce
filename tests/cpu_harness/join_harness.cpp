// join_harness.cpp -- host build of the rules strsim_join.h shares with the join kernels (strsim_join_kernels.h), for
// tests/test_join_cpu.py: g++ compiles the same header.
//   join_replay      join_replay_host of join_sweep_host.h (a wave's count sweep, the counts -> prefix -> 64-bit scan, its fill sweep
//                    and the row sort against brute force, with every check of the protocol) under k_join_lane's own part: the
//                    window, the nearest-first steps and the stop rule over the rank table, a pair yielding the rank of a random
//                    (d, s); reports how many candidates the count sweep visited.
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

#include "join_sweep_host.h"

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

// What k_join_lane adds to the shared sweep, over given Indel distances dist[i * nc + j].
struct RankCase {
    const std::vector<uint32_t> &qlen, &clen;
    const uint32_t *dist;
    uint32_t rlimit;
    double cutoff;
    bool nothing;

    double expected(uint32_t i, uint32_t j) const { return epilogue_indel(dist[(size_t)i * clen.size() + j], qlen[i] + clen[j], 0u); }

    // k_join_lane's loop over the lengths: the wave's window nearest-first, a length no lane needs skipped, the stop after a step
    // none of whose lengths was needed
    void lengths(JoinWave &W, bool fill, uint32_t split) const
    {
        const uint16_t *const rank = table().rank;
        uint32_t lmin = 0xFFFFFFFFu, lmax = 0u;
        for (uint32_t i = 0; i < W.nq; ++i) { lmin = std::min(lmin, qlen[i]); lmax = std::max(lmax, qlen[i]); }
        uint32_t lo, hi;
        extract_window(rank, lmin, lmax, rlimit, lo, hi);
        const uint32_t steps = nearest_steps(lmin, lmax, lo, hi);
        for (uint32_t g = 0; g < steps; ++g) {
            uint32_t first, last, stride;
            if (!nearest_step_range(lmin, lmax, lo, hi, g, first, last, stride)) continue;
            bool needed = false;
            for (uint32_t lc = first; lc <= last; lc += stride) {
                std::vector<uint8_t> need(W.nq);
                bool any = false;
                for (uint32_t i = 0; i < W.nq; ++i) any |= (need[i] = join_needs(rank, qlen[i], lc, rlimit));
                if (!any) continue;
                needed = true;
                join_slice_host(
                    W, fill, split, lc, [&](uint32_t i) { return need[i] != 0; },
                    [&](uint32_t i) { return JoinRankRule{rank + (qlen[i] + lc) * EXTRACT_TAB_W, rlimit, table().rep}; },
                    [&](uint32_t i, uint32_t j) { return dist[(size_t)i * W.nc + j]; });
            }
            if (!needed) break;
        }
    }
    int after(const JoinWave &, bool) const { return 0; }
};

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
    RankCase C{qlen, clen, dist.data(), rlimit, cutoff, rlimit == 0u};
    const uint32_t shift = (uint32_t)(seed % 3u); // groups of 1, 2 and 4 positions
    return join_replay_host(C, nq, clen, upper != 0, splits, undersize, shift, stats);
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
