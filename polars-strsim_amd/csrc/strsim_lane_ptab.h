// strsim_lane_ptab.h -- the Levenshtein lane core with match masks from PER-LANE TABLES IN REGISTERS, read with v_perm_b32.
//
// The bit-plane match mask of strsim_lane_core.h (eq_mask) spends five v_bfe_i32 (half rate) + five v_bitop3_b32 per column.
// Split the 5-bit character c = (h << 3) | e and keep two small tables per pair
//     L[e], e = 0..7: the pattern positions whose low three bits equal e       M[h], h = 0..3: the same for bits 3..4
// so that Eq(c) = L[c & 7] & M[c >> 3].  v_perm_b32 picks any byte of two registers with a per-lane selector, so a table of
// 8 x 32 bits is read one BYTE SLICE at a time: lo[s] / hi[s] hold byte s of L[0..3] / L[4..7], m[s] byte s of M[0..3].  With a
// text dword's four characters as the selector, one v_perm returns byte s of the table entry of all four columns:
//     sel_l = w & 0x07070707, sel_h = (w >> 3) & 0x03030303            (selector bytes stay <= 7: higher values mean constants)
//     Q_s = perm(hi[s], lo[s], sel_l) & perm(., m[s], sel_h)            byte j of Q_s = byte s of Eq(c_j)
// and a 4 x 4 byte transpose of Q_0..3 (eight v_perm) gives the four masks as words: 3 + 8 + 4 + 8 = 23 instructions per four
// columns against 40.  The tables cost 12 v_bitop3 + three byte transposes (24 v_perm) per pair and live in 12 registers; the
// planes are dead once they are built.  They pay from about a dozen columns on, so the kernel chooses per round
// (STRSIM_STAGE_PTAB_MIN, strsim_lane_stage.h).  Five planes only.
#pragma once
#include "strsim_lane_core.h"

namespace strsim {

struct PermTab {
    uint32_t lo[4], hi[4], m[4];
};

// r[s] byte y = w[y] byte s
STRSIM_HD void transpose4x4_bytes(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t (&r)[4])
{
    const uint32_t t0 = perm_b32(w2, w0, 0x05010400u); // [w0.b0, w2.b0, w0.b1, w2.b1]
    const uint32_t t1 = perm_b32(w2, w0, 0x07030602u); // [w0.b2, w2.b2, w0.b3, w2.b3]
    const uint32_t t2 = perm_b32(w3, w1, 0x05010400u);
    const uint32_t t3 = perm_b32(w3, w1, 0x07030602u);
    r[0] = perm_b32(t2, t0, 0x05010400u);
    r[1] = perm_b32(t2, t0, 0x07030602u);
    r[2] = perm_b32(t3, t1, 0x05010400u);
    r[3] = perm_b32(t3, t1, 0x07030602u);
}

// positions where planes (a, b, c) hold the bits (E & 1, E >> 1 & 1, E >> 2 & 1): one minterm of the truth table
template <int E>
STRSIM_HD uint32_t ptab_minterm(uint32_t a, uint32_t b, uint32_t c)
{
    return bitop3<1 << ((E & 1) * 4 + ((E >> 1) & 1) * 2 + ((E >> 2) & 1))>(a, b, c);
}

STRSIM_HD void ptab_build(const uint32_t (&P)[5], PermTab &T)
{
    transpose4x4_bytes(ptab_minterm<0>(P[0], P[1], P[2]), ptab_minterm<1>(P[0], P[1], P[2]), ptab_minterm<2>(P[0], P[1], P[2]),
                       ptab_minterm<3>(P[0], P[1], P[2]), T.lo);
    transpose4x4_bytes(ptab_minterm<4>(P[0], P[1], P[2]), ptab_minterm<5>(P[0], P[1], P[2]), ptab_minterm<6>(P[0], P[1], P[2]),
                       ptab_minterm<7>(P[0], P[1], P[2]), T.hi);
    // (planes 3 and 4; plane 4 stands in for the third input: minterms 0, 1, 6, 7 are the ones with b == c)
    transpose4x4_bytes(ptab_minterm<0>(P[3], P[4], P[4]), ptab_minterm<1>(P[3], P[4], P[4]), ptab_minterm<6>(P[3], P[4], P[4]),
                       ptab_minterm<7>(P[3], P[4], P[4]), T.m);
}

// Eq[j] = the positions where the pattern equals byte j of w (low five bits compared), j = 0..3
STRSIM_HD void ptab_masks(const PermTab &T, uint32_t w, uint32_t (&Eq)[4])
{
    const uint32_t sel_l = w & 0x07070707u, sel_h = (w >> 3) & 0x03030303u;
    uint32_t q[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) q[s] = perm_b32(T.hi[s], T.lo[s], sel_l) & perm_b32(T.m[s], T.m[s], sel_h);
    transpose4x4_bytes(q[0], q[1], q[2], q[3], Eq);
}

// lev_myers32_snap (strsim_lane_core.h) with table masks: the same recurrence, bounds and exec masking, the match masks of four
// columns at a time.  The test against tmax stays every COLS_PER_TEST columns: a round whose bound falls inside a dword has
// computed that dword's four masks and uses the first ones.
template <int NP>
STRSIM_HD uint32_t lev_myers32_ptab(const uint32_t (&wt)[8], uint32_t lt, uint32_t tmin, uint32_t tmax, const uint32_t (&P)[NP],
                                    uint32_t lp)
{
    static_assert(NP == 5, "the register tables split five bits into 3 + 2");
    static_assert(4 % COLS_PER_TEST == 0, "a text dword is a whole number of column groups");
    PermTab T;
    ptab_build(P, T);
    uint32_t Pv = 0xFFFFFFFFu, Mv = 0u;
    uint32_t Eq[4];
    unrolled_until<0, 32 / COLS_PER_TEST>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if ((uint32_t)(COLS_PER_TEST * g) >= tmax) return false;
        if constexpr ((COLS_PER_TEST * g) % 4 == 0) ptab_masks(T, wt[(COLS_PER_TEST * g) >> 2], Eq);
        auto column = [&](int j) {
            const uint32_t E = Eq[j & 3];
            const uint32_t D0 = bitop3<0xBE>((E & Pv) + Pv, Pv, E) | Mv; // (((Eq & Pv) + Pv) ^ Pv) | Eq | Mv
            const uint32_t nHP = bitop3<0x0E>(Mv, D0, Pv);               // ~HP = ~Mv & (D0 | Pv)
            const uint32_t nX = twice(nHP);                               // ~((HP << 1) | 1)
            const uint32_t HN2 = twice(D0 & Pv);                          // HN << 1
            Pv = bitop3<0xF2>(HN2, D0, nX);                               // (HN << 1) | ~(D0 | X)
            Mv = bitop3<0x50>(D0, D0, nX);                                // D0 & X
        };
        if ((uint32_t)(COLS_PER_TEST * (g + 1)) >= tmin) {               // (uniform) some lane's text may end in this group
#pragma unroll
            for (int jj = 0; jj < COLS_PER_TEST; ++jj)
                if ((uint32_t)(COLS_PER_TEST * g + jj) < lt) column(COLS_PER_TEST * g + jj);
        } else {
#pragma unroll
            for (int jj = 0; jj < COLS_PER_TEST; ++jj) column(COLS_PER_TEST * g + jj);
        }
        return true;
    });
    const uint32_t rows = low_ones(lp);
    return lt + popc32(Pv & rows) - popc32(Mv & rows);
}

} // namespace strsim
