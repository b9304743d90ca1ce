// Host build of the shared extract code of strsim_extract.h, for tests/test_extract_cpu.py: g++ compiles the same header.
//   extract_core   what one lane of k_extract_lane computes for a query (the pattern, <= 32 ASCII bytes) against a candidate (the
//                  uniform text, <= 32 bytes): the planes of build_planes and the Indel core, on NP = 5 or 7 planes.
//   extract_tab_*  the rank table the library builds, its scores and the cutoff -> rank-limit conversion.
//   extract_wave   the sweep of one wave of k_extract_lane (one split) over given distances: the same window, nearest-first
//                  order, skip and stop rules and the same list insertion, with the ballots written as loops over the lanes.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <numeric>
#include <vector>

#include "strsim_extract.h"

using namespace strsim;

static void window32(const char *s, uint32_t len, uint32_t (&w)[8])
{
    uint8_t b[32] = {};
    memcpy(b, s, len);
    for (int d = 0; d < 8; ++d) w[d] = (uint32_t)b[4 * d] | ((uint32_t)b[4 * d + 1] << 8) | ((uint32_t)b[4 * d + 2] << 16) | ((uint32_t)b[4 * d + 3] << 24);
}

extern "C" uint32_t extract_core(const char *q, uint32_t lq, const char *c, uint32_t lc, int np)
{
    uint32_t wq[8], wc[8];
    window32(q, lq, wq);
    window32(c, lc, wc);
    if (np == 5) {
        uint32_t P[5];
        build_planes<5>(wq, P);
        return extract_indel_uniform_text<5>(wc, lc, P, lq);
    }
    uint32_t P[7];
    build_planes<7>(wq, P);
    return extract_indel_uniform_text<7>(wc, lc, P, lq);
}

static const ExtractTable &table()
{
    static const ExtractTable *const t = [] {
        ExtractTable *n = new ExtractTable;
        extract_build_table(*n);
        return n;
    }();
    return *t;
}

extern "C" uint32_t extract_tab_nranks() { return table().nranks; }
extern "C" uint32_t extract_tab_rank(uint32_t d, uint32_t s) { return extract_rank(table().rank, d, s); }
extern "C" double extract_tab_score(uint32_t r) { return extract_rank_score(table().rep, r); }
extern "C" uint32_t extract_tab_limit(double cutoff) { return extract_rank_limit(table(), cutoff); }
extern "C" double extract_pair_score(uint32_t d, uint32_t s) { return epilogue_indel(d, s, 0); }

template <int K>
static uint64_t wave(const uint32_t *qlen, uint32_t nq, const uint32_t *clen, uint32_t nc, const uint32_t *dist, double cutoff,
                     uint32_t *out_idx, double *out_score)
{
    const uint16_t *const rank = table().rank;
    const uint32_t rlimit = extract_rank_limit(table(), cutoff);
    std::vector<std::vector<uint64_t>> keys(nq, std::vector<uint64_t>(K, NEAREST_EMPTY));
    // the candidates in length order (any order inside a length: the lists must not depend on it -- here, descending index)
    std::vector<uint32_t> order(nc);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return clen[a] != clen[b] ? clen[a] < clen[b] : a > b; });
    uint64_t visited = 0;
    auto kth = [&](uint32_t i) { return keys[i][K - 1]; };
    if (rlimit) { // (the library launches no sweep when nothing is admissible)
        uint32_t lmin = 0xFFFFFFFFu, lmax = 0u;
        for (uint32_t i = 0; i < nq; ++i) { lmin = std::min(lmin, qlen[i]); lmax = std::max(lmax, qlen[i]); }
        uint32_t lo, hi;
        extract_window(rank, lmin, lmax, rlimit, lo, hi);
        const uint32_t steps = nearest_steps(lmin, lmax, lo, hi);
        for (uint32_t g = 0; g < steps; ++g) {
            uint32_t first, last, stride;
            if (!nearest_step_range(lmin, lmax, lo, hi, g, first, last, stride)) continue;
            bool needed = false;
            for (uint32_t lc = first; lc <= last; lc += stride) {
                auto any_needs = [&] {
                    bool any = false;
                    for (uint32_t i = 0; i < nq; ++i) any |= extract_needs(extract_ub(rank, qlen[i], lc), extract_bound(kth(i), rlimit));
                    return any;
                };
                if (any_needs()) needed = true;
                for (uint32_t x = 0; x < nc; ++x) {
                    const uint32_t j = order[x];
                    if (clen[j] != lc) continue;
                    if (!any_needs()) break;
                    ++visited;
                    for (uint32_t i = 0; i < nq; ++i) {
                        const uint32_t r = extract_rank(rank, dist[(size_t)i * nc + j], qlen[i] + lc);
                        uint64_t (&k)[K] = *reinterpret_cast<uint64_t(*)[K]>(keys[i].data());
                        if (r < rlimit && extract_key(r, j) < k[K - 1]) nearest_insert<K>(k, extract_key(r, j));
                    }
                }
            }
            if (!needed) break;
        }
    }
    for (uint32_t i = 0; i < nq; ++i)
        for (int s = 0; s < K; ++s) {
            const bool e = keys[i][s] == NEAREST_EMPTY;
            out_idx[(size_t)i * K + s] = e ? 0xFFFFFFFFu : (uint32_t)keys[i][s];
            out_score[(size_t)i * K + s] = e ? std::numeric_limits<double>::quiet_NaN() : extract_rank_score(table().rep, (uint32_t)(keys[i][s] >> 32));
        }
    return visited;
}

// Returns the number of candidates the wave computed (out of nc), or ~0 for a K other than 1, 4, 16.
extern "C" uint64_t extract_wave(const uint32_t *qlen, uint32_t nq, const uint32_t *clen, uint32_t nc, const uint32_t *dist, uint32_t K,
                                 double cutoff, uint32_t *out_idx, double *out_score)
{
    if (K == 1) return wave<1>(qlen, nq, clen, nc, dist, cutoff, out_idx, out_score);
    if (K == 4) return wave<4>(qlen, nq, clen, nc, dist, cutoff, out_idx, out_score);
    if (K == 16) return wave<16>(qlen, nq, clen, nc, dist, cutoff, out_idx, out_score);
    return ~0ull;
}

// The static window of a wave under a cutoff: lo, hi (0xFFFFFFFF both when nothing is admissible).
extern "C" void extract_window_h(uint32_t lmin, uint32_t lmax, double cutoff, uint32_t *out)
{
    const uint32_t rlimit = extract_rank_limit(table(), cutoff);
    out[0] = out[1] = 0xFFFFFFFFu;
    if (rlimit) extract_window(table().rank, lmin, lmax, rlimit, out[0], out[1]);
}
