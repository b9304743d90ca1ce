// Host build of the shared nearest-match code of strsim_nearest.h, for tests/test_nearest_cpu.py: g++ compiles the same header.
//   nearest_core  what one lane of k_nearest_lane computes for a query (the pattern, <= 32 ASCII bytes) against a candidate (the
//                 uniform text, <= 32 bytes): the planes of build_planes and the Levenshtein or OSA core, on NP = 5 or 7 planes.
//   nearest_wave  the sweep of one wave of k_nearest_lane (one split) over given distances: sweep_host.h's loop under the
//                 kernel's own NearestRules.
#include "sweep_host.h"

using namespace strsim;

extern "C" uint32_t nearest_core(const char *q, uint32_t lq, const char *c, uint32_t lc, int np, int tr)
{
    uint32_t wq[8], wc[8];
    window32(q, lq, wq);
    window32(c, lc, wc);
    if (np == 5) {
        uint32_t P[5];
        build_planes<5>(wq, P);
        return tr ? nearest_osa_uniform_text<5>(wc, lc, P, lq) : nearest_lev_uniform_text<5>(wc, lc, P, lq);
    }
    uint32_t P[7];
    build_planes<7>(wq, P);
    return tr ? nearest_osa_uniform_text<7>(wc, lc, P, lq) : nearest_lev_uniform_text<7>(wc, lc, P, lq);
}

template <int K>
static uint64_t wave(const uint32_t *qlen, uint32_t nq, const uint32_t *clen, uint32_t nc, const uint32_t *dist, uint32_t kmax,
                     uint32_t *out_idx, uint32_t *out_d)
{
    std::vector<SweepKeys<K>> keys = sweep_empty<K>(nq);
    const uint64_t visited = sweep_wave<NearestRules<false>, K>(NearestRules<false>{kmax}, qlen, nq, clen, nc, dist, keys); // (no rule depends on TR)
    for (uint32_t i = 0; i < nq; ++i)
        for (int s = 0; s < K; ++s) {
            out_idx[(size_t)i * K + s] = (uint32_t)keys[i].k[s];
            out_d[(size_t)i * K + s] = (uint32_t)(keys[i].k[s] >> 32);
        }
    return visited;
}

// Returns the number of candidates the wave computed (out of nc), or ~0 for a K other than 1, 4, 16.
extern "C" uint64_t nearest_wave(const uint32_t *qlen, uint32_t nq, const uint32_t *clen, uint32_t nc, const uint32_t *dist, uint32_t K,
                                 uint32_t kmax, uint32_t *out_idx, uint32_t *out_d)
{
    if (K == 1) return wave<1>(qlen, nq, clen, nc, dist, kmax, out_idx, out_d);
    if (K == 4) return wave<4>(qlen, nq, clen, nc, dist, kmax, out_idx, out_d);
    if (K == 16) return wave<16>(qlen, nq, clen, nc, dist, kmax, out_idx, out_d);
    return ~0ull;
}

// The window and the step ranges as the kernel sees them: lo, hi, steps, then (first, last, stride, any) for each step.
extern "C" void nearest_plan(uint32_t lmin, uint32_t lmax, uint32_t kmax, uint32_t *out)
{
    uint32_t lo, hi;
    nearest_window(lmin, lmax, kmax, lo, hi);
    const uint32_t steps = nearest_steps(lmin, lmax, lo, hi);
    out[0] = lo; out[1] = hi; out[2] = steps;
    for (uint32_t g = 0; g < steps; ++g) {
        uint32_t f = 0, l = 0, s = 0;
        const bool any = nearest_step_range(lmin, lmax, lo, hi, g, f, l, s);
        out[3 + 4 * g] = f; out[4 + 4 * g] = l; out[5 + 4 * g] = s; out[6 + 4 * g] = any;
    }
}

extern "C" int nearest_needs_h(uint32_t lq, uint32_t lc, uint64_t kth, uint32_t kmax) { return nearest_needs(lq, lc, nearest_bound(kth, kmax)); }
