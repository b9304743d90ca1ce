// Host build of the bounded-distance code of strsim_distance.h, for tests/test_distance_cpu.py: g++ compiles the same header.
//   dist_lane_distance  what one lane of k_dist_lane computes for an ASCII pair of <= 64 bytes (prefilter, recurrence, clamp);
//   dist_block_distance what one wave of k_dist_wave computes for a pair of scalar-value strings (prefilter, the block cutoff
//                       over dist_column, the early end, the clamp), with the match words built by a loop instead of a ballot.
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

// p: the pattern (lp <= 64), t: the text (lt <= 64); wide as k_dist_lane picks it from the wave's longest pattern.
extern "C" uint32_t dist_lane_distance(const char *p, uint32_t lp, const char *t, uint32_t lt, uint32_t tmax, int wide, int tr,
                                       uint32_t k)
{
    if (dist_lane_row(true, lp, lt, true, k) == DIST_ROW_CUT) return k + 1u;
    uint32_t wp[16], wt[16], Plo[7], Phi[7];
    window64(p, lp, wp);
    window64(t, lt, wt);
    osa_planes(wp, Plo, Phi, wide != 0);
    uint32_t d;
    if (tr) d = wide ? dist_lane_core<uint64_t, true>(wt, lt, tmax, Plo, Phi, lp) : dist_lane_core<uint32_t, true>(wt, lt, tmax, Plo, Phi, lp);
    else d = wide ? dist_lane_core<uint64_t, false>(wt, lt, tmax, Plo, Phi, lp) : dist_lane_core<uint32_t, false>(wt, lt, tmax, Plo, Phi, lp);
    return dist_clamp(d, k);
}

// k_dist_lane's class of a row (DistRow): live, the two byte lengths, whether both strings are ASCII
extern "C" uint32_t dist_lane_class(int live, uint32_t la, uint32_t lb, int ascii, uint32_t k)
{
    return dist_lane_row(live != 0, la, lb, ascii != 0, k);
}

template <bool TR>
static uint64_t block_run(const uint32_t *pat, uint32_t m, const uint32_t *txt, uint32_t nt, uint32_t k, uint64_t *columns,
                          uint64_t *words)
{
    const uint32_t W = (m + 63u) / 64u;
    const bool bounded = k < nt;
    std::vector<uint32_t> P((size_t)W * 64u, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < m; ++i) P[i] = pat[i];
    std::vector<DistWord> st(W);
    int y = dist_first_y(W, m, k, bounded);
    for (uint32_t w = 0; w < W; ++w) st[w] = dist_word_start<DistWord>(w);
    uint64_t c = 0;
    for (uint32_t j = 0; j < nt; ++j) {
        const uint32_t ch = txt[j];
        dist_column<TR>(st.data(), y, W, k, c, bounded, [&](uint32_t w) {
            ++*words; // (one match word per word step)
            uint64_t e = 0;
            for (int l = 0; l < 64; ++l) e |= (uint64_t)(P[64u * w + l] == ch) << l;
            return e;
        });
        ++c;
        if (y < 0 && c > k) { *columns = c; return (uint64_t)k + 1u; }
    }
    *columns = c;
    return dist_final(st.data(), y, W, m, nt, k);
}

// *columns: the text columns run before the pair was decided (the early end of the cutoff shows here); *words: the word steps
// those columns took (the work the cutoff trims inside a column)
extern "C" uint32_t dist_block_distance(const uint32_t *a, uint32_t la, const uint32_t *b, uint32_t lb, int tr, uint32_t k,
                                        uint64_t *columns, uint64_t *words)
{
    const bool a_is_pat = la <= lb;
    const uint32_t *pat = a_is_pat ? a : b, *txt = a_is_pat ? b : a;
    const uint32_t m = a_is_pat ? la : lb, nt = a_is_pat ? lb : la;
    *columns = 0;
    *words = 0;
    if (dist_length_cut(m, nt, k)) return k + 1u;
    if (m == 0) return dist_clamp(nt, k);
    const uint64_t d = tr ? block_run<true>(pat, m, txt, nt, k, columns, words) : block_run<false>(pat, m, txt, nt, k, columns, words);
    return dist_clamp(d, k);
}
