// Host build of the partial-ratio cores of strsim_partial.h, for tests/test_partial_cpu.py: g++ compiles the same header, the
// test drives it pair by pair against tests/partial_ref.py.  partial_lane_host is what k_partial_lane runs per lane (table, first
// direction, second direction for equal lengths, the choice between them); partial_wave_host the per-window cores of
// k_partial_wave (the 64-bit table form for needles of up to 64 values, the word form beyond).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "strsim_partial.h"

using namespace strsim;

// a, b: ASCII bytes, at most 32 each.  mmax / nmax / m2max: the bounds "the wave" runs (>= this pair's needle, haystack, and needle
// again for the second direction); second_any: another lane of the wave has equal lengths, so the second pass runs although this
// pair may take no part in it.  out: score bits are returned; span[4].  Returns 0 on a bad argument.
extern "C" int partial_lane_host(const char *a, uint32_t la, const char *b, uint32_t lb, uint32_t mmax, uint32_t nmax, uint32_t m2max,
                                 int second_any, double *score, uint32_t *span)
{
    if (la > 32u || lb > 32u) return 0;
    const bool a_needle = la <= lb;
    const uint32_t m = a_needle ? la : lb, n = a_needle ? lb : la;
    if (mmax < m || nmax < n || mmax > 32u || nmax > 32u || m2max > 32u) return 0;
    uint8_t nb[32] = {}, hb[32] = {};
    memcpy(nb, a_needle ? a : b, m);
    memcpy(hb, a_needle ? b : a, n);
    uint32_t wn[8], wh[8];
    memcpy(wn, nb, 32);
    memcpy(wh, hb, 32);
    uint32_t tab[32];
    for (int j = 0; j < 32; ++j) tab[j] = 0xDEADBEEFu; // (columns >= nmax are never written and must never be read)
    partial_lane_table(wn, wh, m, n, nmax, tab, 1u);
    uint32_t V0;
    PartialWin best = partial_lane_first<true>(tab, 1u, m, n, mmax, nmax, V0);
    bool second = false;
    const bool both = m != 0u && la == lb;
    if (both || second_any) {
        const uint32_t m2 = both ? m : 0u;
        if (m2max < m2) return 0;
        const PartialWin b2 = partial_lane_second<true>(tab, 1u, m2, m2max, V0);
        second = both && partial_gt(b2.l, b2.wl, best.l, best.wl, m);
        if (second) best = b2;
    }
    if (m == 0u) {
        *score = n == 0u ? 1.0 : 0.0;
        span[0] = span[1] = span[2] = span[3] = 0u;
        return 1;
    }
    *score = partial_score(best, m);
    const uint32_t ws = best.start, we = ws + best.wl;
    if (a_needle && !second) { span[0] = 0u; span[1] = la; span[2] = ws; span[3] = we; }
    else { span[0] = ws; span[1] = we; span[2] = 0u; span[3] = lb; }
    return 1;
}

// P(s, t) for scalar values, 1 <= m <= n, by the wave tier's cores: out3 = l, window length, start.
extern "C" int partial_wave_host(const uint32_t *s, uint32_t m, const uint32_t *t, uint32_t n, uint32_t *out3)
{
    if (m == 0u || n < m) return 0;
    PartialWin best = partial_floor();
    if (m <= 64u) {
        std::vector<uint64_t> tab(n);
        for (uint32_t j = 0; j < n; ++j) {
            uint64_t e = 0;
            for (uint32_t i = 0; i < m; ++i) e |= (uint64_t)(s[i] == t[j]) << i;
            tab[j] = e;
        }
        // "lanes": the prefix round, then the window starting at every position
        for (uint32_t lane = 0; lane + 1u < m; ++lane) {
            const PartialWin c{partial_window_lcs64(tab.data(), 0u, lane + 1u, m, m), lane + 1u, 0u};
            if (partial_before(c, best, m)) best = c;
        }
        for (uint32_t start = n; start-- > 0u;) { // (backwards: the total order, not the walk, must decide)
            const uint32_t len = m < n - start ? m : n - start;
            const PartialWin c{partial_window_lcs64(tab.data(), start, len, m, m), len, start};
            if (partial_before(c, best, m)) best = c;
        }
    } else {
        const uint32_t W = (m + 63u) / 64u;
        std::vector<uint32_t> pat((size_t)W * 64u, 0xFFFFFFFFu);
        for (uint32_t i = 0; i < m; ++i) pat[i] = s[i];
        std::vector<uint64_t> V(W);
        best = partial_words_windows(
            t, m, n, [&] { for (uint32_t w = 0; w < W; ++w) V[w] = ~0ull; },
            [&](uint32_t ch) {
                partial_words_column(
                    [&](uint32_t w) {
                        uint64_t e = 0;
                        for (uint32_t i = 0; i < 64u; ++i) e |= (uint64_t)(pat[64u * w + i] == ch) << i;
                        return e;
                    },
                    V.data(), W);
            },
            [&] { return partial_words_lcs(V.data(), W, m); });
    }
    out3[0] = best.l; out3[1] = best.wl; out3[2] = best.start;
    return 1;
}

extern "C" double partial_score_host(uint32_t l, uint32_t wl, uint32_t m) { return partial_score(PartialWin{l, wl, 0u}, m); }
extern "C" uint64_t partial_wave_words_host(uint64_t m, uint64_t n) { return partial_wave_words(m, n); }
