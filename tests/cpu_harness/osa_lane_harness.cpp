// Host build of the OSA recurrences as the similarity runs them (strsim_osa.h, strsim_distance.h), for tests/test_osa_cpu.py: g++
// compiles the same headers, the test drives them pair by pair against tests/osa_ref.py.
//   osa_lane_distance   what one lane of k_dist_lane<true, LIT, double> computes for an ASCII pair of <= 64 bytes;
//   osa_words_distance  what one wave of k_dist_wave<true, double> computes for a pair of scalar-value strings (dist_column without
//                       a cutoff over osa_word_step, then dist_final), with the match words built by a loop instead of a ballot.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "strsim_distance.h"

using namespace strsim;

static void window64(const char *s, uint32_t len, uint32_t (&w)[16])
{
    uint8_t b[64] = {};
    memcpy(b, s, len);
    for (int d = 0; d < 16; ++d) w[d] = (uint32_t)b[4 * d] | ((uint32_t)b[4 * d + 1] << 8) | ((uint32_t)b[4 * d + 2] << 16) | ((uint32_t)b[4 * d + 3] << 24);
}

// OSA distance of pattern p (lp <= 64 ASCII bytes) and text t (lt <= 64), with the 32-bit masks when wide == 0 (lp <= 32).
// tmax >= lt: the columns the wave runs (a longer text of another lane); the state must not move beyond lt.
extern "C" uint32_t osa_lane_distance(const char *p, uint32_t lp, const char *t, uint32_t lt, uint32_t tmax, int wide)
{
    uint32_t wp[16], wt[16], Plo[7], Phi[7];
    window64(p, lp, wp);
    window64(t, lt, wt);
    osa_planes(wp, Plo, Phi, wide != 0);
    return wide ? dist_lane_core<uint64_t, true>(wt, lt, tmax, Plo, Phi, lp) : dist_lane_core<uint32_t, true>(wt, lt, tmax, Plo, Phi, lp);
}

extern "C" double osa_lane_score(uint32_t d, uint32_t la, uint32_t lb) { return epilogue_osa(d, la, lb); }

// p: the pattern (m scalar values; the kernel takes the string with fewer of them), t: the text (n values).
extern "C" uint64_t osa_words_distance(const uint32_t *p, uint32_t m, const uint32_t *t, uint32_t n)
{
    if (m == 0u) return n;
    const uint32_t W = (m + 63u) / 64u;
    std::vector<uint32_t> pat((size_t)W * 64u, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < m; ++i) pat[i] = p[i];
    std::vector<DistWordFree> state(W);
    for (uint32_t w = 0; w < W; ++w) state[w] = dist_word_start<DistWordFree>(w);
    int y = dist_first_y(W, m, DIST_UNBOUNDED, false);
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t ch = t[j];
        dist_column<true>(state.data(), y, W, DIST_UNBOUNDED, j, false, [&](uint32_t w) {
            uint64_t e = 0;
            for (int l = 0; l < 64; ++l) e |= (uint64_t)(pat[64u * w + l] == ch) << l;
            return e;
        });
    }
    return dist_final(state.data(), y, W, m, n, DIST_UNBOUNDED);
}
