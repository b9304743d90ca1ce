// CPU harness for polars-strsim_amd/csrc/strsim_lane_ptab.h: the Levenshtein lane core with match masks from per-lane register
// tables (v_perm_b32 through its host fallback) against lev_myers32_snap and the textbook DP.  Test infrastructure only.
#include <cstdint>
#include <cstring>
#include <algorithm>
#include "strsim_lane_core.h"
#include "strsim_lane_ptab.h"

using namespace strsim;

static uint32_t dp_distance(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb)
{
    uint32_t row[33];
    for (uint32_t j = 0; j <= lb; ++j) row[j] = j;
    for (uint32_t i = 1; i <= la; ++i) {
        uint32_t diag = row[0];
        row[0] = i;
        for (uint32_t j = 1; j <= lb; ++j) {
            const uint32_t sub = diag + (a[i - 1] != b[j - 1] ? 1u : 0u);
            diag = row[j];
            row[j] = std::min(sub, std::min(row[j], row[j - 1]) + 1u);
        }
    }
    return row[lb];
}

// One pair: wa / wb are whole 32-byte windows (the bytes at and behind the lengths are whatever the caller put there), the text
// is wa (lt bytes), the pattern wb (lp bytes), 1 <= lt, lp <= 32.  Runs every bound the kernel can hand the core for this text:
// tmax = every even value in [lt, 32], tmin = every value in [1, lt].  out = {runs, first failing tmin, tmax, ptab, snap, dp}.
// Returns the number of runs in which the three distances were not all equal.
extern "C" int harness_ptab_sweep(const uint8_t *wa32, uint32_t lt, const uint8_t *wb32, uint32_t lp, uint32_t *out)
{
    uint32_t wa[8], wb[8];
    std::memcpy(wa, wa32, 32);
    std::memcpy(wb, wb32, 32);
    const uint32_t dp = dp_distance(wa32, lt, wb32, lp);
    uint32_t P[5];
    build_planes<5>(wb, P);
    int bad = 0;
    uint32_t runs = 0;
    for (uint32_t tmax = (lt + 1u) & ~1u; tmax <= 32u; tmax += 2u)
        for (uint32_t tmin = 1u; tmin <= lt; ++tmin) {
            const uint32_t dt = lev_myers32_ptab<5>(wa, lt, tmin, tmax, P, lp);
            const uint32_t ds = lev_myers32_snap<5>(wa, lt, tmin, tmax, P, lp);
            ++runs;
            if (dt != ds || dt != dp) {
                if (!bad) { out[1] = tmin; out[2] = tmax; out[3] = dt; out[4] = ds; out[5] = dp; }
                ++bad;
            }
        }
    out[0] = runs;
    return bad;
}

// The tables of a 32-byte pattern window against eq_mask<5>, for all 32 five-bit characters: entry by entry (L[c & 7] and
// M[c >> 3] put together from their byte slices) and through ptab_masks with c in each of a dword's four bytes, the other
// three bytes holding other characters with high bits set.  0 = all agree.
extern "C" int harness_ptab_tables(const uint8_t *wb32)
{
    uint32_t wb[8];
    std::memcpy(wb, wb32, 32);
    uint32_t P[5];
    build_planes<5>(wb, P);
    PermTab T;
    ptab_build(P, T);
    for (uint32_t c = 0; c < 32u; ++c) {
        const uint32_t ref = eq_mask<5>(P, 0xFFFFFFFFu, c, 0);
        uint32_t def = 0; // the definition, from the bytes
        for (int i = 0; i < 32; ++i) def |= (uint32_t)((wb32[i] & 31u) == c) << i;
        if (def != ref) return 1000 + (int)c;
        const uint32_t e = c & 7u, h = c >> 3;
        uint32_t L = 0, M = 0;
        for (int s = 0; s < 4; ++s) {
            L |= (((e < 4u ? T.lo[s] : T.hi[s]) >> (8u * (e & 3u))) & 0xFFu) << (8 * s);
            M |= ((T.m[s] >> (8u * h)) & 0xFFu) << (8 * s);
        }
        uint32_t Lref = 0, Mref = 0;
        for (int i = 0; i < 32; ++i) {
            Lref |= (uint32_t)((wb32[i] & 7u) == e) << i;
            Mref |= (uint32_t)(((wb32[i] >> 3) & 3u) == h) << i;
        }
        if (L != Lref) return 2000 + (int)c;
        if (M != Mref) return 3000 + (int)c;
        if ((L & M) != ref) return 4000 + (int)c;
        for (int j = 0; j < 4; ++j) {
            uint32_t w = 0;
            for (int q = 0; q < 4; ++q) {
                const uint32_t other = 0xE0u | ((c * 7u + 5u * (uint32_t)q + 1u) & 31u);
                w |= (q == j ? (0x60u | c) : other) << (8 * q);
            }
            uint32_t Eq[4];
            ptab_masks(T, w, Eq);
            for (int q = 0; q < 4; ++q)
                if (Eq[q] != eq_mask<5>(P, 0xFFFFFFFFu, w, q)) return 5000 + 100 * j + (int)c;
        }
    }
    return 0;
}
