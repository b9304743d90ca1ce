// strsim_osa.h -- optimal string alignment (restricted Damerau-Levenshtein) similarity, measure id 6 (STRSIM_OSA).
//
// osa(a, b) = 1.0 when a == b or both are empty, else 1.0 - (d / max(|a|, |b|)) with d the OSA distance over Unicode scalar
// values: the Levenshtein DP plus one transposition term, D[i-2][j-2] + 1 when a_i = b_{j-1} and a_{i-1} = b_j.  No substring
// is edited twice, so this is NOT the unrestricted Damerau-Levenshtein distance (("ca", "abc") is 3 here, 2 there).
//
// Bit-parallel form (Hyyro 2003): Myers' recurrence with, per column j of the text,
//   TR = ((~D0_{j-1} & Eq_j) << 1) & Eq_{j-1}
//   D0 = (((Eq & VP) + VP) ^ VP) | Eq | VN | TR
// and the usual HP / HN / VP / VN update.  The distance is read off the last column: lt + popc(VP & rows) - popc(VN & rows).
//
// This header holds the recurrence and what the kernels of several measures build on: the single-word step and its match mask
// (osa_step, osa_eq, osa_planes), the word step of a longer pattern with its four carries (osa_word_step), the 64-byte window
// loads (osa_load64, osa_high_bits) and the epilogue.  The kernels are those of the edit distances (strsim_distance.h): the
// similarity is k_dist_lane<true, LIT, double> and k_dist_wave<true, double>.
#pragma once
#include <stdint.h>

#include "strsim_lane_core.h"
#include "strsim_wave_util.h"

namespace strsim {

constexpr int OSA = 6;                        // = STRSIM_OSA
constexpr uint32_t OSA_LANE_MAX_BYTES = 64u;  // k_dist_lane: both strings ASCII and at most this long
constexpr uint32_t OSA_WAVE_LDS_CPS = 2048u;  // the wave kernels: patterns up to this many scalar values live in LDS

STRSIM_HD uint32_t osa_popc(uint32_t x) { return popc32(x); }
STRSIM_HD uint32_t osa_popc(uint64_t x) { return popc32((uint32_t)x) + popc32((uint32_t)(x >> 32)); }

// One column of the recurrence on a single mask word (the pattern fits it).  D0p / EQp: D0 and Eq of the previous column
// (zero before the first, so that TR is zero there).  Rows above the pattern only ever influence rows above them.
template <typename T>
STRSIM_HD void osa_step(T Eq, T &VP, T &VN, T &D0p, T &EQp)
{
    const T TR = ((~D0p & Eq) << 1) & EQp;
    const T D0 = (((Eq & VP) + VP) ^ VP) | Eq | VN | TR;
    const T HP = VN | ~(D0 | VP);
    const T HN = D0 & VP;
    const T X = (HP << 1) | (T)1;
    VP = (HN << 1) | ~(D0 | X);
    VN = D0 & X;
    D0p = D0;
    EQp = Eq;
}

// Match mask of byte `byte` (0..3, static) of dword w against the pattern's seven planes: bytes 0..31 in Plo, 32..63 in Phi.
template <typename T>
STRSIM_HD T osa_eq(const uint32_t (&Plo)[7], const uint32_t (&Phi)[7], uint32_t w, int byte)
{
    const uint32_t lo = eq_mask<7>(Plo, 0xFFFFFFFFu, w, byte);
    if constexpr (sizeof(T) == 4) {
        (void)Phi;
        return lo;
    } else {
        return ((uint64_t)eq_mask<7>(Phi, 0xFFFFFFFFu, w, byte) << 32) | lo;
    }
}

// Seven bit-planes of the 64-byte pattern window w (bytes 0..31 -> Plo, 32..63 -> Phi).
STRSIM_HD void osa_planes(const uint32_t (&w)[16], uint32_t (&Plo)[7], uint32_t (&Phi)[7], bool hi)
{
    uint32_t h[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) h[d] = w[d];
    build_planes<7>(h, Plo);
    if (hi) {
#pragma unroll
        for (int d = 0; d < 8; ++d) h[d] = w[8 + d];
        build_planes<7>(h, Phi);
    } else {
#pragma unroll
        for (int k = 0; k < 7; ++k) Phi[k] = 0u;
    }
}

// strsim.rs:127-130 and :160 with the OSA distance: both empty -> 1.0 (a == b gives d = 0 -> 1.0 by the formula itself)
STRSIM_HD double epilogue_osa(uint64_t dist, uint64_t la, uint64_t lb)
{
    if (la == 0 && lb == 0) return 1.0;
    return epilogue_levenshtein(dist, la, lb);
}

// One column of the recurrence on one 64-row word of a longer pattern, for dist_column of strsim_distance.h (TR = false: Myers'
// step, D0p / EQp / tr_c are left alone).  The words of a column are advanced low to high with four carries between them: add_c of the add, hp_c / hn_c the bits HP << 1 and HN << 1 shift in (1 and 0 into word 0: the
// top boundary row grows by one a column; on return the horizontal delta of the word's bottom row), tr_c the bit of ~D0p & Eq
// that the TR term shifts in.  All four start a column as 0, 1, 0, 0.
template <bool TR>
STRSIM_HD void osa_word_step(uint64_t Eq, uint64_t &VP, uint64_t &VN, uint64_t &D0p, uint64_t &EQp, uint64_t &add_c, uint64_t &hp_c,
                             uint64_t &hn_c, uint64_t &tr_c)
{
    const uint64_t vp = VP, vn = VN;
    uint64_t TRw = 0ull;
    if constexpr (TR) {
        const uint64_t t = ~D0p & Eq;
        TRw = ((t << 1) | tr_c) & EQp;
        tr_c = t >> 63;
    }
    const uint64_t x = Eq & vp;
    const uint64_t s1 = x + vp;
    const uint64_t s2 = s1 + add_c;
    add_c = (uint64_t)(s1 < x) | (uint64_t)(s2 < s1);
    const uint64_t D0 = (s2 ^ vp) | Eq | vn | TRw;
    const uint64_t HP = vn | ~(D0 | vp);
    const uint64_t HN = D0 & vp;
    const uint64_t X = (HP << 1) | hp_c;
    hp_c = HP >> 63;
    const uint64_t Y = (HN << 1) | hn_c;
    hn_c = HN >> 63;
    VP = Y | ~(D0 | X);
    VN = D0 & X;
    if constexpr (TR) {
        D0p = D0;
        EQp = Eq;
    }
}

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

// 64 bytes of vals[off, off + len) into w[0..15] (len <= 64); nothing outside the string is read, the rest is zero.
__device__ __forceinline__ void osa_load64(const uint8_t *__restrict__ vals, uint32_t off, uint32_t len, uint32_t (&w)[16])
{
    uint32_t a[8], b[8];
    load_window32(vals, off, off + len, a);
    if (len > 32u) {
        load_window32(vals, off + 32u, off + len, b);
    } else {
#pragma unroll
        for (int d = 0; d < 8; ++d) b[d] = 0u;
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) { w[d] = a[d]; w[8 + d] = b[d]; }
}

__device__ __forceinline__ uint32_t osa_high_bits(const uint32_t (&w)[16])
{
    uint32_t o = 0u;
#pragma unroll
    for (int d = 0; d < 16; ++d) o |= w[d];
    return o & 0x80808080u;
}

#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
