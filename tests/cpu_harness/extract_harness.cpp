// Host build of the shared extract code of strsim_extract.h, for tests/test_extract_cpu.py: g++ compiles the same header.
//   extract_core   what one lane of k_extract_lane computes for a query (the pattern, <= 32 ASCII bytes) against a candidate (the
//                  uniform text, <= 32 bytes): the planes of build_planes and the Indel core, on NP = 5 or 7 planes.
//   extract_tab_*  the rank table the library builds, its scores and the cutoff -> rank-limit conversion.
//   extract_wave   the sweep of one wave of k_extract_lane (one split) over given distances: sweep_host.h's loop under the
//                  kernel's own ExtractRules.
#include <limits>

#include "strsim_extract.h"
#include "sweep_host.h"

using namespace strsim;

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
    const ExtractRules R{table().rank, table().rep, extract_rank_limit(table(), cutoff)};
    std::vector<SweepKeys<K>> keys = sweep_empty<K>(nq);
    // (the library launches no sweep when nothing is admissible)
    const uint64_t visited = R.rlimit ? sweep_wave<ExtractRules, K>(R, qlen, nq, clen, nc, dist, keys) : 0;
    for (uint32_t i = 0; i < nq; ++i)
        for (int s = 0; s < K; ++s) {
            const bool e = keys[i].k[s] == NEAREST_EMPTY;
            out_idx[(size_t)i * K + s] = e ? 0xFFFFFFFFu : (uint32_t)keys[i].k[s];
            out_score[(size_t)i * K + s] = e ? std::numeric_limits<double>::quiet_NaN() : R.score(keys[i].k[s]);
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
