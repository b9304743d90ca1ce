// strsim_partial.h -- partial ratio (best-window Indel similarity) and its alignment, measure id 10 (STRSIM_PARTIAL_RATIO).
//
// Over Unicode scalar values.  For a needle s (m = |s| >= 1) and a haystack t (n = |t| >= m) the windows of t are the proper
// prefixes t[0:w] (w = 1 .. m-1), every substring of length m, and the proper suffixes t[i:n] (i = n-m+1 .. n-1): n + m - 1 of them.
// P(s, t) is the maximum of indel(s, window) (epilogue_indel of strsim_indel.h) over the windows; ties go to the window with the
// smallest end, then the smallest start.  partial_ratio(a, b) = P(shorter, longer); for equal lengths max(P(a, b), P(b, a)) with a
// the needle unless b as the needle is strictly better; 1.0 when both are empty, 0.0 when exactly one is.
//
// The needle is the pattern of the bit-parallel LCS (strsim_indel.h): Eq[j], the needle positions equal to haystack character j,
// is built ONCE per pair.  A sweep from start i sets V to all ones and runs columns i, i + 1, ...; after w columns
// popcount(~V & rows) = LCS(s, t[i:i+w]).  The sweep from 0 read after every column gives the prefixes and the first full window,
// the sweep from each i >= 1 run for min(m, n - i) columns the full window or suffix that starts there.  1.0 - d / (m + w) is
// monotone in 2 l / (m + w), so windows are compared by integer cross-multiplication and the f64 epilogue runs once, for the winner.
// For |a| = |b| the second direction costs one more sweep: the zero bits of V among rows < r count LCS(a[0:r], b), so the sweep
// over all of b already holds b against every prefix of a, and the same sweep over the reversed strings holds every suffix.
//
// Two tiers, both finished in stream order (the protocol of k_indel_lane / k_indel_wave):
//   k_partial_lane<LIT, ALIGN>  one pair per lane, both strings ASCII and <= 32 bytes.  Eq[] lives in LDS as [column][thread]
//                               (conflict-free ds_read_b32 / ds_write_b32, 32 KB per workgroup of 256, no barrier: a lane reads
//                               only what it wrote).  Loop bounds are wave maxima in scalar registers, lanes past their own end
//                               are masked.  Every other row is appended to the work list.
//   k_partial_wave<ALIGN>       one pair per wave for the work list: any UTF-8, any length.  Needles of up to 64 values: a table of
//                               one 64-bit mask per haystack character (compare + ballot), then lane i sweeps the window that
//                               starts at 64 round + i, and the wave reduces the lane winners by the total order.  Longer needles:
//                               V in several words, the windows one after the other (O(n m ceil(m / 64)) word steps, not tuned).
//                               Tables beyond PARTIAL_WAVE_LDS_WORDS words live in the context's scratch.
// ALIGN adds the winner's start to the running best and the 16-byte span store.
#pragma once
#include <stdint.h>

#include "strsim_indel.h"

namespace strsim {

constexpr int PARTIAL_RATIO = 10;                    // = STRSIM_PARTIAL_RATIO
constexpr uint32_t PARTIAL_LANE_MAX_BYTES = 32u;     // k_partial_lane: both strings ASCII and at most this long
constexpr uint32_t PARTIAL_WAVE_LDS_WORDS = 4096u;   // k_partial_wave: 32-bit words of LDS a pair's tables may take

// A window of the haystack and its LCS with the needle: [start, start + wl).
struct PartialWin {
    uint32_t l, wl, start;
};
// The first window in the tie order with no match at all: a lower bound of every pair's answer (it IS the answer when nothing
// matches: window t[0:1]).
STRSIM_HD PartialWin partial_floor() { return PartialWin{0u, 1u, 0u}; }

// 2 l / (m + wl) of c strictly above that of b
STRSIM_HD bool partial_gt(uint32_t cl, uint32_t cwl, uint32_t bl, uint32_t bwl, uint32_t m)
{
    return (uint64_t)cl * ((uint64_t)m + bwl) > (uint64_t)bl * ((uint64_t)m + cwl);
}
// the total order: c goes before b when it scores higher, or the same with the smaller end, or the same end and the smaller start
STRSIM_HD bool partial_before(const PartialWin &c, const PartialWin &b, uint32_t m)
{
    const uint64_t x = (uint64_t)c.l * ((uint64_t)m + b.wl), y = (uint64_t)b.l * ((uint64_t)m + c.wl);
    if (x != y) return x > y;
    const uint64_t ce = (uint64_t)c.start + c.wl, be = (uint64_t)b.start + b.wl;
    if (ce != be) return ce < be;
    return c.start < b.start;
}

STRSIM_HD double partial_score(const PartialWin &w, uint32_t m)
{
    return epilogue_indel((uint64_t)m + w.wl - 2ull * w.l, m, w.wl);
}

STRSIM_HD uint32_t partial_brev32(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x);
#else
    uint32_t r = 0u;
    for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i);
    return r;
#endif
}

// ---- the lane tier's core (one pair, needle and haystack of at most 32 ASCII bytes) ----

// the 32-bit column step of indel_lane_step on a ready-made mask
STRSIM_HD void partial_step32(uint32_t e, uint32_t &V)
{
    const uint32_t u = V & e;
    V = (V + u) | (V & ~e);
}

// The walk visits the windows in the tie order, so "first strict maximum" is the rule.
template <bool ALIGN>
STRSIM_HD void partial_consider(PartialWin &best, bool on, uint32_t l, uint32_t wl, uint32_t start, uint32_t m)
{
    // (l <= 32 and m + wl <= 64: 32-bit products)
    const bool take = on && l * (m + best.wl) > best.l * (m + wl);
    best.l = take ? l : best.l;
    best.wl = take ? wl : best.wl;
    if constexpr (ALIGN) best.start = take ? start : best.start;
}

// Eq[] of the pair into tab[column * stride], columns 0 .. nmax - 1 (nmax >= n, at most 32): needle bytes in wn, haystack bytes in
// wh, zero past the ends.  Zero padding never matches: needle rows >= m are masked out, and columns >= n are all zero (a zero
// column leaves V alone), so a NUL byte is a character like any other.
STRSIM_HD void partial_lane_table(const uint32_t (&wn)[8], const uint32_t (&wh)[8], uint32_t m, uint32_t n, uint32_t nmax,
                                  uint32_t *tab, uint32_t stride)
{
    uint32_t P[7];
    build_planes<7>(wn, P);
    const uint32_t rows = low_ones(m);
    unrolled_until<0, 32>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if ((uint32_t)j >= nmax) return false;
        tab[(uint32_t)j * stride] = eq_mask<7>(P, (uint32_t)j < n ? rows : 0u, wh[j >> 2], j & 3);
        return true;
    });
}

// Every window of the haystack (n >= m, m >= 1) against the needle.  mmax >= m, nmax >= n: the bounds the wave runs (its longest
// needle and haystack); a lane with m = 0 comes back with partial_floor().  V0: V after the sweep from 0, for partial_lane_second.
template <bool ALIGN>
STRSIM_HD PartialWin partial_lane_first(const uint32_t *tab, uint32_t stride, uint32_t m, uint32_t n, uint32_t mmax, uint32_t nmax,
                                        uint32_t &V0)
{
    const uint32_t rows = low_ones(m);
    PartialWin best = partial_floor();
    // the sweep from 0: t[0:w + 1] after column w -- the proper prefixes, then the first full window at w + 1 = m
    uint32_t V = 0xFFFFFFFFu;
    const uint32_t c0 = mmax < nmax ? mmax : nmax;
    for (uint32_t w = 0u; w < c0; ++w) {
        partial_step32(tab[w * stride] & bit_fill(rows, (int)w), V); // (bit w of rows: w < m)
        partial_consider<ALIGN>(best, w < m, popc32(~V & rows), w + 1u, 0u, m);
    }
    V0 = V;
    // the sweep from i: the full window t[i:i + m], or the suffix t[i:n] once it is shorter than m
    for (uint32_t i = 1u; i < nmax; ++i) {
        V = 0xFFFFFFFFu;
        const uint32_t cols = mmax < nmax - i ? mmax : nmax - i;
        for (uint32_t w = 0u; w < cols; ++w) partial_step32(tab[(i + w) * stride] & bit_fill(rows, (int)w), V);
        const bool on = i < n;
        const uint32_t left = on ? n - i : 0u;
        partial_consider<ALIGN>(best, on, popc32(~V & rows), m < left ? m : left, i, m);
    }
    return best;
}

// |a| = |b| = m >= 1, the second direction: b is the needle and the windows are those of a, from the table built with a as the
// needle.  V0 (a swept over all of b) holds LCS(a[0:r], b) in its rows < r; the same sweep over the reversed strings -- column k is
// the bit reversal of column m - 1 - k -- holds LCS(a[m - r:m], b).  m2 = m for a lane that takes part, 0 for one that does not;
// mmax >= m2.
template <bool ALIGN>
STRSIM_HD PartialWin partial_lane_second(const uint32_t *tab, uint32_t stride, uint32_t m2, uint32_t mmax, uint32_t V0)
{
    PartialWin best = partial_floor();
    for (uint32_t r = 1u; r <= mmax; ++r) // the proper prefixes a[0:r], then all of a
        partial_consider<ALIGN>(best, r <= m2, popc32(~V0 & low_ones(r)), r, 0u, m2);
    uint32_t V = 0xFFFFFFFFu;
    const uint32_t sh = (32u - m2) & 31u;
    for (uint32_t k = 0u; k < mmax; ++k) {
        const bool on = k < m2;
        const uint32_t e = partial_brev32(tab[(on ? m2 - 1u - k : 0u) * stride]) >> sh;
        partial_step32(on ? e : 0u, V);
    }
    for (uint32_t i = 1u; i < mmax; ++i) { // the proper suffixes a[i:m]
        const bool on = i < m2;
        const uint32_t r = on ? m2 - i : 0u;
        partial_consider<ALIGN>(best, on, popc32(~V & low_ones(r)), r, i, m2);
    }
    return best;
}

// ---- the wave tier's per-window cores ----

// LCS of a needle of m <= 64 values with the window [start, start + len) of the haystack, from the table of 64-bit masks.  The
// loop runs `cols` >= len columns (the wave's: m); the columns past the window are not read.
STRSIM_HD uint32_t partial_window_lcs64(const uint64_t *tab, uint32_t start, uint32_t len, uint32_t cols, uint32_t m)
{
    uint64_t V = ~0ull;
    for (uint32_t w = 0u; w < cols; ++w) {
        const uint64_t e = w < len ? tab[start + w] : 0ull;
        const uint64_t u = V & e;
        V = (V + u) | (V & ~e);
    }
    const uint64_t rows = m >= 64u ? ~0ull : ((1ull << m) - 1ull);
    return osa_popc((uint64_t)(~V & rows));
}

// One column over the W words of a long needle: eq(w) is the match mask of word w for the column's character.
template <typename EqWord>
STRSIM_HD void partial_words_column(EqWord eq, uint64_t *V, uint32_t W)
{
    uint64_t c = 0ull;
    for (uint32_t w = 0u; w < W; ++w) {
        uint64_t v = V[w];
        indel_word_step(eq(w), v, c);
        V[w] = v;
    }
}
STRSIM_HD uint32_t partial_words_lcs(const uint64_t *V, uint32_t W, uint32_t m)
{
    uint32_t l = 0u;
    for (uint32_t w = 0u; w < W; ++w) l += indel_word_lcs(V[w], w, m);
    return l;
}

// Every window of a haystack of n values against a needle of m values (any m >= 1, n >= m), one after the other in the tie order.
// column(ch) advances V by the haystack value ch; reset() sets V to all ones; lcs() reads it.  hay: the haystack's values.
template <typename Reset, typename Column, typename Lcs>
STRSIM_HD PartialWin partial_words_windows(const uint32_t *hay, uint32_t m, uint32_t n, Reset reset, Column column, Lcs lcs)
{
    PartialWin best = partial_floor();
    reset();
    for (uint32_t w = 0u; w < m; ++w) {
        column(hay[w]);
        const PartialWin c{lcs(), w + 1u, 0u};
        if (partial_before(c, best, m)) best = c;
    }
    for (uint32_t i = 1u; i < n; ++i) {
        reset();
        const uint32_t len = m < n - i ? m : n - i;
        for (uint32_t w = 0u; w < len; ++w) column(hay[i + w]);
        const PartialWin c{lcs(), len, i};
        if (partial_before(c, best, m)) best = c;
    }
    return best;
}

// 32-bit words of table space k_partial_wave needs for a needle of m and a haystack of n values: n 64-bit masks (m <= 64), or the
// haystack's values, the needle's values padded to whole words of 64, and one 64-bit V per word (at an even offset).
STRSIM_HD uint64_t partial_wave_words(uint64_t m, uint64_t n)
{
    if (m <= 64u) return 2u * n;
    const uint64_t W = (m + 63u) / 64u;
    return ((n + 64u * W + 1u) & ~(uint64_t)1) + 2u * W;
}

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

typedef uint32_t partial_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ void partial_store(double *__restrict__ out, uint32_t *__restrict__ span, uint64_t row, double score,
                                              uint32_t as, uint32_t ae, uint32_t bs, uint32_t be)
{
    out[row] = score;
    if (span) {
        partial_u32x4 v;
        v.x = as; v.y = ae; v.z = bs; v.w = be;
        *reinterpret_cast<partial_u32x4 *>(span + 4u * row) = v;
    }
}

// One pair per lane.  LIT: 0 = row against row, 1 = a is a literal (rowsA == 1), 2 = b is; which of the two is the needle still
// depends on each row's length, so a literal is loaded like a row (every lane reads the same address).  Rows this kernel cannot
// take are appended to `worklist` (worklist_append<true> of strsim_wave_util.h: st->wave_rows, st->max_len bounds their needles,
// st->pad1[0] their haystacks, in bytes).  The status block is zeroed before the launch.  ALIGN: span != nullptr.
template <int LIT, bool ALIGN>
__global__ __launch_bounds__(256) void k_partial_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA,
                                                      const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t nrows,
                                                      double *__restrict__ out, uint32_t *__restrict__ span,
                                                      uint32_t *__restrict__ worklist, DevStatus *st)
{
    __shared__ uint32_t s_eq[PARTIAL_LANE_MAX_BYTES * 256u]; // [column][thread]
    const auto [row, live, a0, la, b0, lb] = lane_row(offA, offB, nrows, LIT == 1, LIT == 2);
    const bool fits = live && la <= PARTIAL_LANE_MAX_BYTES && lb <= PARTIAL_LANE_MAX_BYTES;
    const bool a_needle = la <= lb;
    // a lane that does not fit loads nothing and runs no column
    const uint32_t m = fits ? (a_needle ? la : lb) : 0u, n = fits ? (a_needle ? lb : la) : 0u;
    uint32_t wn[8], wh[8];
    {
        const uint8_t *nv = a_needle ? valA : valB, *hv = a_needle ? valB : valA;
        const uint32_t no = a_needle ? a0 : b0, ho = a_needle ? b0 : a0;
        load_window32(nv, no, no + m, wn);
        load_window32(hv, ho, ho + n, wh);
    }
    uint32_t hi = 0u;
#pragma unroll
    for (int d = 0; d < 8; ++d) hi |= wn[d] | wh[d];
    // wave-uniform, in scalar registers
    const uint32_t mmax = indel_wave_max(m), nmax = indel_wave_max(n);
    uint32_t *tab = s_eq + threadIdx.x;
    partial_lane_table(wn, wh, m, n, nmax, tab, 256u);
    uint32_t V0;
    PartialWin best = partial_lane_first<ALIGN>(tab, 256u, m, n, mmax, nmax, V0);
    bool second = false;
    const bool both = m != 0u && la == lb;
    if (__ballot(both) != 0ull) {
        const uint32_t m2 = both ? m : 0u;
        const PartialWin b2 = partial_lane_second<ALIGN>(tab, 256u, m2, indel_wave_max(m2), V0);
        second = both && partial_gt(b2.l, b2.wl, best.l, best.wl, m);
        if (second) best = b2;
    }
    const bool ok = fits && (hi & 0x80808080u) == 0u;
    worklist_append<true>(live && !ok, row, la, lb, worklist, st); // rows for k_partial_wave
    if (ok) {
        if (m == 0u) {
            partial_store(out, ALIGN ? span : nullptr, row, n == 0u ? 1.0 : 0.0, 0u, 0u, 0u, 0u);
        } else {
            const double score = partial_score(best, m);
            const uint32_t ws = ALIGN ? best.start : 0u, we = ws + best.wl;
            if (a_needle && !second) partial_store(out, ALIGN ? span : nullptr, row, score, 0u, la, ws, we);
            else partial_store(out, ALIGN ? span : nullptr, row, score, ws, we, 0u, lb);
        }
    }
}

// the lane winners of a wave, reduced by the total order (every lane ends with the wave's)
__device__ __forceinline__ PartialWin partial_wave_reduce(PartialWin best, uint32_t m)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        PartialWin o;
        o.l = (uint32_t)__shfl_xor((int)best.l, s, 64);
        o.wl = (uint32_t)__shfl_xor((int)best.wl, s, 64);
        o.start = (uint32_t)__shfl_xor((int)best.start, s, 64);
        if (partial_before(o, best, m)) best = o;
    }
    return best;
}

// P(needle, haystack) of one pair by the wave (m >= 1, n >= m scalar values); mem: partial_wave_words(m, n) words, 8-byte aligned;
// s_pat: 64 words of LDS.  Every lane returns the winner.
__device__ __forceinline__ PartialWin partial_wave_pair(const uint8_t *__restrict__ pp, uint32_t pbytes, uint32_t m,
                                                        const uint8_t *__restrict__ tp, uint32_t tbytes, uint32_t n, uint32_t *mem,
                                                        uint32_t *s_pat, uint32_t lane)
{
    PartialWin best = partial_floor();
    if (m <= 64u) {
        wave_decode(pp, pbytes, s_pat, lane);
        __syncthreads();
        const uint32_t pv = lane < m ? s_pat[lane] : 0xFFFFFFFFu; // (no scalar value is 0xFFFFFFFF)
        uint64_t *tab = reinterpret_cast<uint64_t *>(mem);
        uint32_t pos = 0u;
        wave_each_char(tp, tbytes, lane, [&](uint32_t ch) {
            const uint64_t e = (uint64_t)__ballot(pv == ch);
            if (lane == 0u) tab[pos] = e;
            ++pos;
        });
        __syncthreads();
        // the proper prefixes: lane i takes t[0:i + 1]
        if (m >= 2u) {
            const bool on = lane + 1u < m;
            const uint32_t len = on ? lane + 1u : 0u;
            const PartialWin c{partial_window_lcs64(tab, 0u, len, m, m), len, 0u};
            if (on && partial_before(c, best, m)) best = c;
        }
        // lane i of round r takes the window that starts at 64 r + i
        for (uint32_t r0 = 0u; r0 < n; r0 += 64u) {
            const uint32_t start = r0 + lane;
            const bool on = start < n;
            const uint32_t left = on ? n - start : 0u;
            const uint32_t len = m < left ? m : left;
            const PartialWin c{partial_window_lcs64(tab, on ? start : 0u, len, m, m), len, start};
            if (on && partial_before(c, best, m)) best = c;
        }
        best = partial_wave_reduce(best, m);
    } else {
        const uint32_t W = (m + 63u) / 64u;
        uint32_t *hay = mem, *pat = mem + n;
        uint64_t *V = reinterpret_cast<uint64_t *>(mem + ((n + 64u * W + 1u) & ~1u));
        wave_decode(tp, tbytes, hay, lane);
        wave_pattern(pp, pbytes, m, W, pat, lane);
        __syncthreads();
        // (every lane stores the same V words and reads back its own store)
        best = partial_words_windows(
            hay, m, n, [&] { for (uint32_t w = 0u; w < W; ++w) V[w] = ~0ull; },
            [&](uint32_t ch) { partial_words_column([&](uint32_t w) { return (uint64_t)__ballot(pat[64u * w + lane] == ch); }, V, W); },
            [&] { return partial_words_lcs(V, W, m); });
    }
    __syncthreads(); // (the next pair overwrites s_pat and mem)
    return best;
}

// One pair per wave (blockDim.x = 64) for the rows k_partial_lane put on the work list (st->wave_rows of them).  The string with
// fewer scalar values is the needle; for equal counts both directions run.  scratch: gridDim.x slots of slot_words words for the
// pairs whose tables take more than PARTIAL_WAVE_LDS_WORDS words (nullptr when the call has none).
template <bool ALIGN>
__global__ __launch_bounds__(64) void k_partial_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                     const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                                     double *__restrict__ out, uint32_t *__restrict__ span,
                                                     const uint32_t *__restrict__ worklist, const DevStatus *st, uint32_t *scratch,
                                                     uint64_t slot_words)
{
    __shared__ uint64_t s_mem[PARTIAL_WAVE_LDS_WORDS / 2u];
    __shared__ uint32_t s_pat[64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = st->wave_rows;
    for (uint32_t r = blockIdx.x; r < count; r += gridDim.x) {
        const auto [row, pa, pb, na, nb, ca, cb] = wave_pair(offA, valA, rowsA, offB, valB, rowsB, worklist[r]);
        if (ca == 0u || cb == 0u) {
            if (lane == 0u) partial_store(out, ALIGN ? span : nullptr, row, (ca | cb) == 0u ? 1.0 : 0.0, 0u, 0u, 0u, 0u);
            continue;
        }
        const bool a_needle = ca <= cb;
        const uint32_t m = a_needle ? ca : cb, n = a_needle ? cb : ca;
        uint32_t *mem = reinterpret_cast<uint32_t *>(s_mem);
        if (partial_wave_words(m, n) > PARTIAL_WAVE_LDS_WORDS) mem = scratch + (uint64_t)blockIdx.x * slot_words;
        PartialWin best = a_needle ? partial_wave_pair(pa, na, m, pb, nb, n, mem, s_pat, lane)
                                   : partial_wave_pair(pb, nb, m, pa, na, n, mem, s_pat, lane);
        bool second = false;
        if (ca == cb) {
            const PartialWin b2 = partial_wave_pair(pb, nb, m, pa, na, n, mem, s_pat, lane);
            second = partial_gt(b2.l, b2.wl, best.l, best.wl, m);
            if (second) best = b2;
        }
        if (lane == 0u) {
            const double score = partial_score(best, m);
            const uint32_t ws = best.start, we = ws + best.wl;
            if (a_needle && !second) partial_store(out, ALIGN ? span : nullptr, row, score, 0u, ca, ws, we);
            else partial_store(out, ALIGN ? span : nullptr, row, score, ws, we, 0u, cb);
        }
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
