// The sweep of one wave of the length-ordered lane kernels (search_sweep_lane of strsim_nearest_kernels.h, one split) on the
// host, over given distances and under the rule objects the kernels run (NearestRules of strsim_nearest.h, ExtractRules of
// strsim_extract.h): the same loop, with a ballot written as a loop over the lanes and the wave minimum / maximum as std::min /
// std::max.  Shared by nearest_harness.cpp and extract_harness.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "strsim_nearest.h"

// The first 32 bytes of a string as the eight words of k_match_pack (zeros behind the string).
inline void window32(const char *s, uint32_t len, uint32_t (&w)[8])
{
    uint8_t b[32] = {};
    memcpy(b, s, len);
    for (int d = 0; d < 8; ++d) w[d] = (uint32_t)b[4 * d] | ((uint32_t)b[4 * d + 1] << 8) | ((uint32_t)b[4 * d + 2] << 16) | ((uint32_t)b[4 * d + 3] << 24);
}

template <int K>
struct SweepKeys {
    uint64_t k[K];
};

// The empty lists of nq queries.
template <int K>
std::vector<SweepKeys<K>> sweep_empty(uint32_t nq)
{
    SweepKeys<K> e;
    std::fill(e.k, e.k + K, strsim::NEAREST_EMPTY);
    return std::vector<SweepKeys<K>>(nq, e);
}

// nq <= 64 queries of lengths qlen against nc candidates of lengths clen, dist[i * nc + j] the distance of pair (i, j), into
// the (empty) lists `keys`; returns the number of candidates the wave computed (out of nc).
template <class Rules, int K>
uint64_t sweep_wave(const Rules &R, const uint32_t *qlen, uint32_t nq, const uint32_t *clen, uint32_t nc, const uint32_t *dist,
                    std::vector<SweepKeys<K>> &keys)
{
    using namespace strsim;
    // the candidates in length order (any order inside a length: the lists must not depend on it -- here, descending index)
    std::vector<uint32_t> order(nc);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return clen[a] != clen[b] ? clen[a] < clen[b] : a > b; });
    uint64_t visited = 0;
    uint32_t lmin = 0xFFFFFFFFu, lmax = 0u;
    for (uint32_t i = 0; i < nq; ++i) { lmin = std::min(lmin, qlen[i]); lmax = std::max(lmax, qlen[i]); }
    uint32_t lo, hi;
    R.window(lmin, lmax, lo, hi);
    const uint32_t steps = nearest_steps(lmin, lmax, lo, hi);
    for (uint32_t g = 0; g < steps; ++g) {
        if constexpr (Rules::STOP_BY_BOUND) {
            uint32_t maxb = 0;
            for (uint32_t i = 0; g && i < nq; ++i) maxb = std::max(maxb, R.bound(keys[i].k[K - 1]));
            if (g && R.done(g, maxb)) break;
        }
        uint32_t first, last, stride;
        if (!nearest_step_range(lmin, lmax, lo, hi, g, first, last, stride)) continue;
        [[maybe_unused]] bool needed = false;
        for (uint32_t lc = first; lc <= last; lc += stride) {
            auto any_needs = [&] {
                bool any = false;
                for (uint32_t i = 0; i < nq; ++i) any |= R.needs(qlen[i], R.at(qlen[i], lc), keys[i].k[K - 1]);
                return any;
            };
            if constexpr (!Rules::STOP_BY_BOUND)
                if (any_needs()) needed = true;
            for (uint32_t x = 0; x < nc; ++x) {
                const uint32_t j = order[x];
                if (clen[j] != lc) continue;
                if (!any_needs()) break;
                ++visited;
                for (uint32_t i = 0; i < nq; ++i) {
                    bool ok;
                    const uint64_t key = R.key(dist[(size_t)i * nc + j], R.at(qlen[i], lc), j, ok);
                    if (ok && key < keys[i].k[K - 1]) nearest_insert<K>(keys[i].k, key);
                }
            }
        }
        if constexpr (!Rules::STOP_BY_BOUND)
            if (!needed) break;
    }
    return visited;
}
