// Host build of the Indel (LCS) recurrences of strsim_indel.h, for tests/test_indel_cpu.py: g++ compiles the same header, the
// test drives it pair by pair against tests/indel_ref.py.  indel_lane_lcs_w is what k_indel_lane runs per lane at W mask words,
// indel_words_lcs the 64-bit word step of k_indel_wave (register and LDS form alike).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "strsim_indel.h"

using namespace strsim;

template <int W>
static uint32_t lane_lcs(const char *p, uint32_t lp, const char *t, uint32_t lt, uint32_t tmax, bool masked)
{
    uint8_t pb[32 * W] = {}, tb[128] = {};
    memcpy(pb, p, lp);
    memcpy(tb, t, lt);
    uint32_t P[W][7];
    for (int w = 0; w < W; ++w) {
        uint32_t win[8];
        memcpy(win, pb + 32 * w, 32);
        build_planes<7>(win, P[w]);
    }
    uint32_t V[W];
    for (int w = 0; w < W; ++w) V[w] = 0xFFFFFFFFu;
    for (uint32_t h = 0; 64u * h < tmax; ++h) {
        uint32_t wt[16];
        memcpy(wt, tb + 64 * h, 64);
        if (masked) indel_lane_half<W, true>(wt, h, lt, tmax, P, V);
        else indel_lane_half<W, false>(wt, h, lt, tmax, P, V);
    }
    return indel_lane_lcs<W>(V, lp);
}

// LCS of pattern p (lp <= 32 W ASCII bytes) and text t (lt <= 128), with W mask words.  tmax >= lt: the columns the wave runs (a
// longer text of another lane); masked = 0 is the literal form (tmax == lt).  0xFFFFFFFF: the pattern does not fit W words.
extern "C" uint32_t indel_lane_lcs_w(const char *p, uint32_t lp, const char *t, uint32_t lt, uint32_t tmax, int W, int masked)
{
    if (lp > 32u * (uint32_t)W || lt > 128u || tmax > 128u) return 0xFFFFFFFFu;
    switch (W) {
    case 1: return lane_lcs<1>(p, lp, t, lt, tmax, masked != 0);
    case 2: return lane_lcs<2>(p, lp, t, lt, tmax, masked != 0);
    case 3: return lane_lcs<3>(p, lp, t, lt, tmax, masked != 0);
    case 4: return lane_lcs<4>(p, lp, t, lt, tmax, masked != 0);
    default: return 0xFFFFFFFFu;
    }
}

// LCS of pattern p (m scalar values) and text t (n values) by the 64-bit word step, padded to `words` words (>= ceil(m / 64)).
extern "C" uint32_t indel_words_lcs(const uint32_t *p, uint32_t m, const uint32_t *t, uint32_t n, uint32_t words)
{
    std::vector<uint32_t> pat((size_t)words * 64u, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < m; ++i) pat[i] = p[i];
    std::vector<uint64_t> V(words, ~0ull);
    for (uint32_t j = 0; j < n; ++j) {
        uint64_t c = 0;
        for (uint32_t w = 0; w < words; ++w) {
            uint64_t Eq = 0;
            for (uint32_t i = 0; i < 64u; ++i) Eq |= (uint64_t)(pat[64u * w + i] == t[j]) << i;
            indel_word_step(Eq, V[w], c);
        }
    }
    uint32_t l = 0;
    for (uint32_t w = 0; w < words; ++w)
        if (m > 64u * w) l += indel_word_lcs(V[w], w, m);
    return l;
}

extern "C" double indel_score(uint64_t d, uint64_t la, uint64_t lb) { return epilogue_indel(d, la, lb); }
extern "C" uint32_t indel_clamp(uint64_t d, uint32_t k) { return dist_clamp(d, k); }
extern "C" int indel_length_cut(uint32_t la, uint32_t lb, uint32_t k) { return dist_length_cut(la, lb, k) ? 1 : 0; }
