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
// Two tiers, both finished in stream order:
//   k_osa_lane<LIT>  one pair per lane, both strings ASCII and <= 64 bytes; the pattern in seven bit-planes of 32 or 64 bits
//                    (eq_mask of strsim_lane_core.h), the text walked byte by byte from registers.  Every other row is
//                    appended to a work list (worklist_append of strsim_wave_util.h).
//   k_osa_wave       one pair per wave for the work list: any UTF-8, any length.  Both strings are decoded to scalar values;
//                    the shorter (in scalar values) is the pattern, held in LDS up to OSA_WAVE_LDS_CPS values and in the
//                    context's scratch above that.  The match words of a text character are built 64 pattern values at a
//                    time by a compare and a ballot; the words are then advanced one after the other with the four carries
//                    between them (the add, HP << 1, HN << 1 and the TR << 1 term): osa_word_step, which k_dist_wave
//                    (strsim_distance.h) runs too.  The row set-up, the decode and the text walk are strsim_wave_util.h's.
#pragma once
#include <stdint.h>

#include "strsim_lane_core.h"
#include "strsim_wave_util.h"

namespace strsim {

constexpr int OSA = 6;                        // = STRSIM_OSA
constexpr uint32_t OSA_LANE_MAX_BYTES = 64u;  // k_osa_lane: both strings ASCII and at most this long
constexpr uint32_t OSA_WAVE_LDS_CPS = 2048u;  // k_osa_wave: patterns up to this many scalar values live in LDS

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

// OSA distance of an ASCII pattern (lp <= 32 for T = uint32_t, <= 64 for uint64_t; planes from build_planes<7>) against the
// text in wt (lt <= 64 bytes).  Columns tmax and beyond are not run (lane-uniform, >= lt); columns lt .. tmax-1 leave the
// state alone.
template <typename T>
STRSIM_HD uint32_t osa_lane_core(const uint32_t (&wt)[16], uint32_t lt, uint32_t tmax, const uint32_t (&Plo)[7],
                                 const uint32_t (&Phi)[7], uint32_t lp)
{
    T VP = ~(T)0, VN = 0, D0p = 0, EQp = 0;
    unrolled_until<0, 64>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if ((uint32_t)j >= tmax) return false;
        if ((uint32_t)j < lt) osa_step<T>(osa_eq<T>(Plo, Phi, wt[j >> 2], j & 3), VP, VN, D0p, EQp);
        return true;
    });
    const T rows = lp >= 8 * sizeof(T) ? ~(T)0 : (((T)1 << lp) - (T)1);
    return lt + osa_popc((T)(VP & rows)) - osa_popc((T)(VN & rows));
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

// Scratch of one k_osa_wave wave for patterns of up to m scalar values: the values (padded to whole words of 64) and four
// 64-bit state words per mask word.
STRSIM_HD uint64_t osa_wave_slot_words(uint64_t m)
{
    const uint64_t words = (m + 63u) / 64u;
    return words * 64u + words * 8u;
}

// One column of the recurrence on one 64-row word of a longer pattern, for k_osa_wave (TR = true) and dist_column of
// strsim_distance.h (TR = false: Myers' step, D0p / EQp / tr_c are left alone).  The words of a column are advanced low to high
// with four carries between them: add_c of the add, hp_c / hn_c the bits HP << 1 and HN << 1 shift in (1 and 0 into word 0: the
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

// k_osa_wave's state: four 64-bit words per mask word -- VP, VN, and D0 and Eq of the previous column.
STRSIM_HD void osa_words_init(uint64_t *sw)
{
    sw[0] = ~0ull;
    sw[1] = 0ull;
    sw[2] = 0ull;
    sw[3] = 0ull;
}

// One text column over the W words of that state; eq(w): the match word of pattern word w against the column's character.
template <typename EqFn>
STRSIM_HD void osa_words_column(uint64_t *state, uint32_t W, EqFn &&eq)
{
    uint64_t add_c = 0ull, hp_c = 1ull, hn_c = 0ull, tr_c = 0ull;
    for (uint32_t w = 0; w < W; ++w) {
        const uint64_t Eq = eq(w);
        uint64_t *sw = state + 4 * w;
        uint64_t VP = sw[0], VN = sw[1], D0p = sw[2], EQp = sw[3];
        osa_word_step<true>(Eq, VP, VN, D0p, EQp, add_c, hp_c, hn_c, tr_c);
        sw[0] = VP;
        sw[1] = VN;
        sw[2] = D0p;
        sw[3] = EQp;
    }
}

// The distance after the last of nt columns: the text length plus the vertical deltas of the m pattern rows.
STRSIM_HD uint64_t osa_words_final(const uint64_t *state, uint32_t W, uint32_t m, uint32_t nt)
{
    uint64_t up = 0u, dn = 0u;
    for (uint32_t w = 0; w < W; ++w) {
        const uint32_t r = m - 64u * w;
        const uint64_t rows = r >= 64u ? ~0ull : ((1ull << r) - 1ull);
        up += (uint64_t)osa_popc((uint64_t)(state[4 * w] & rows));
        dn += (uint64_t)osa_popc((uint64_t)(state[4 * w + 1] & rows));
    }
    return nt + up - dn;
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

// One pair per lane.  LIT: 0 = row against row, 1 = a is a literal (rowsA == 1), 2 = b is.  With a literal the literal is the
// text -- the same bytes in every lane, read through a wave-uniform address -- and the row string is the pattern; otherwise the
// longer string is the pattern and the shorter one the text (fewer columns; OSA is symmetric).  Rows this kernel cannot take
// are appended to `worklist`; st->wave_rows counts them and st->max_len bounds their patterns (min of the two byte lengths).
// The status block is zeroed before the launch.
template <int LIT>
__global__ __launch_bounds__(256) void k_osa_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA,
                                                  const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t n,
                                                  double *__restrict__ out, uint32_t *__restrict__ worklist, DevStatus *st)
{
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = row < n;
    const uint64_t ia = (LIT == 1 || !live) ? 0 : row, ib = (LIT == 2 || !live) ? 0 : row;
    const uint32_t a0 = offA[ia], la = offA[ia + 1] - a0;
    const uint32_t b0 = offB[ib], lb = offB[ib + 1] - b0;
    bool ok = live && la <= OSA_LANE_MAX_BYTES && lb <= OSA_LANE_MAX_BYTES;
    // pattern / text choice
    const bool a_is_pat = LIT == 1 ? false : (LIT == 2 ? true : la >= lb);
    const uint8_t *pv = a_is_pat ? valA : valB, *tv = a_is_pat ? valB : valA;
    const uint32_t po = a_is_pat ? a0 : b0, to = a_is_pat ? b0 : a0;
    const uint32_t lp = a_is_pat ? la : lb, lt = a_is_pat ? lb : la;
    uint32_t wp[16] = {}, wt[16] = {};
    if (ok) {
        osa_load64(pv, po, lp, wp);
        osa_load64(tv, to, lt, wt);
        ok = (osa_high_bits(wp) | osa_high_bits(wt)) == 0u;
    }
    worklist_append<false>(live && !ok, row, la, lb, worklist, st); // rows for k_osa_wave
    if (__ballot(ok) == 0ull) return;
    const uint32_t tmax = osa_wave_max(ok ? lt : 0u);
    const uint32_t pmax = osa_wave_max(ok ? lp : 0u);
    uint32_t Plo[7], Phi[7];
    osa_planes(wp, Plo, Phi, pmax > 32u);
    uint32_t d;
    if (pmax <= 32u) d = osa_lane_core<uint32_t>(wt, lt, tmax, Plo, Phi, lp);
    else d = osa_lane_core<uint64_t>(wt, lt, tmax, Plo, Phi, lp);
    if (ok) out[row] = epilogue_osa(d, la, lb);
}

// One pair per wave (blockDim.x = 64) for the rows k_osa_lane put on the work list (st->wave_rows of them).  scratch: gridDim.x
// slots of slot_words words, for patterns of more than OSA_WAVE_LDS_CPS values (nullptr when the call has none).
__global__ __launch_bounds__(64) void k_osa_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                 const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                                 double *__restrict__ out, const uint32_t *__restrict__ worklist,
                                                 const DevStatus *st, uint32_t *scratch, uint64_t slot_words)
{
    __shared__ uint32_t s_pat[OSA_WAVE_LDS_CPS];
    __shared__ uint64_t s_state[4 * (OSA_WAVE_LDS_CPS / 64u)];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = st->wave_rows;
    for (uint32_t k = blockIdx.x; k < count; k += gridDim.x) {
        const auto [row, pa, pb, na, nb, ca, cb] = wave_pair(offA, valA, rowsA, offB, valB, rowsB, worklist[k]);
        const bool a_is_pat = ca <= cb;
        const uint8_t *pp = a_is_pat ? pa : pb, *tp = a_is_pat ? pb : pa;
        const uint32_t pbytes = a_is_pat ? na : nb, tbytes = a_is_pat ? nb : na;
        const uint32_t m = a_is_pat ? ca : cb, nt = a_is_pat ? cb : ca;
        uint64_t d = nt;
        if (m != 0u) {
            const uint32_t W = (m + 63u) / 64u;
            uint32_t *pat = s_pat;
            uint64_t *state = s_state;
            if (m > OSA_WAVE_LDS_CPS) {
                pat = scratch + (uint64_t)blockIdx.x * slot_words;
                state = reinterpret_cast<uint64_t *>(pat + (uint64_t)W * 64u);
            }
            // the pattern's values; those past m never match (no scalar value is 0xFFFFFFFF)
            wave_decode(pp, pbytes, pat, lane);
            for (uint32_t i = m + lane; i < W * 64u; i += 64u) pat[i] = 0xFFFFFFFFu;
            for (uint32_t w = lane; w < W; w += 64u) osa_words_init(state + 4 * w);
            __syncthreads();
            wave_each_char(tp, tbytes, lane, [&](uint32_t c) {
                osa_words_column(state, W, [&](uint32_t w) { return (uint64_t)__ballot(pat[64u * w + lane] == c); });
            });
            d = osa_words_final(state, W, m, nt);
            __syncthreads(); // (the next row overwrites pat / state)
        }
        if (lane == 0u) out[row] = epilogue_osa(d, ca, cb);
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
