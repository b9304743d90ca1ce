// strsim_indel.h -- Indel (longest-common-subsequence) similarity and distance, measure id 8 (STRSIM_INDEL).
//
// Over Unicode scalar values, with l = LCS(a, b):  d = |a| + |b| - 2 l  (insertions and deletions only: a substitution costs 2),
// indel(a, b) = 1.0 when |a| + |b| == 0, else 1.0 - (d / (|a| + |b|)) -- rapidfuzz's Indel.normalized_similarity, fuzz.ratio / 100.
// The distance form writes d when d <= k and k + 1 otherwise (dist_clamp of strsim_distance.h).
//
// Bit-parallel form (Crochemore et al. 2001, Hyyro 2004): V is all ones before the first column; per text character
//   u = V & Eq;  V = (V + u) | (V & ~Eq)
// and l = popcount(~V & rows) after the last.  Between the words of a long pattern only the carry of the add passes upward.
//
// Two tiers, both finished in stream order:
//   k_indel_lane<LIT>  one pair per lane, both strings ASCII and <= 128 bytes.  The longer string is the pattern: seven bit-planes
//                      of W 32-bit words each (build_planes<7> per 32-byte window), W = 1..4 chosen per wave from the wave's
//                      longest pattern; V is W registers and the carry is chained through them.  The text is walked from
//                      registers in two 64-byte halves; a literal is the text of every lane and is held in scalar registers.
//                      Every other row is appended to a work list.
//   k_indel_wave       one pair per wave for the work list: any UTF-8, any length.  Patterns of up to INDEL_WAVE_REG_CPS scalar
//                      values keep their values (one per lane and word) and V in registers: a column is one compare + ballot and
//                      one add-with-carry per word, nothing goes through memory.  Longer patterns hold values and V in LDS up to
//                      OSA_WAVE_LDS_CPS values and in the context's scratch above that.
// Both kernels serve both outputs: out32 != nullptr selects the clamped uint32 distance, else the f64 similarity goes to out64.
#pragma once
#include <stdint.h>

#include "strsim_distance.h"

namespace strsim {

constexpr int INDEL = 8;                          // = STRSIM_INDEL
constexpr uint32_t INDEL_LANE_MAX_BYTES = 128u;   // k_indel_lane: both strings ASCII and at most this long
constexpr uint32_t INDEL_WAVE_REG_CPS = 256u;     // k_indel_wave: patterns up to this many scalar values live in registers

// 1.0 - d / (la + lb) with exactly these two f64 operations (NOT 2 l / (la + lb): the two differ in the last bit)
STRSIM_HD double epilogue_indel(uint64_t d, uint64_t la, uint64_t lb)
{
    if (la + lb == 0) return 1.0;
    return 1.0 - ((double)d / (double)(la + lb));
}

// s = a + b + c (c = 0 or 1), the carry out back in c.  On the device this is v_add_co / v_addc_co.
STRSIM_HD uint32_t indel_addc(uint32_t a, uint32_t b, uint32_t &c)
{
#if defined(__clang__)
    unsigned int co;
    const uint32_t s = __builtin_addc(a, b, c, &co);
    c = co;
    return s;
#else
    const uint64_t s = (uint64_t)a + b + c;
    c = (uint32_t)(s >> 32);
    return (uint32_t)s;
#endif
}

// One column over the W 32-bit words of a lane's pattern, low to high, the carry of the add chained through them.
template <int W>
STRSIM_HD void indel_lane_step(const uint32_t (&Eq)[W], uint32_t (&V)[W])
{
    uint32_t c = 0u;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t u = V[w] & Eq[w];
        V[w] = indel_addc(V[w], u, c) | (V[w] & ~Eq[w]);
    }
}

// Columns 64 h .. 64 h + 63 of the text (its bytes in wt, zero past the end) against the planes P of the pattern.  Columns at or
// beyond tmax are not run (wave-uniform, >= lt); columns lt .. tmax - 1 see no match, which leaves V alone.  MASKED = false: every
// lane whose result is used has lt == tmax (a literal text), and the test per column is left out.
template <int W, bool MASKED>
STRSIM_HD void indel_lane_half(const uint32_t (&wt)[16], uint32_t h, uint32_t lt, uint32_t tmax, const uint32_t (&P)[W][7],
                               uint32_t (&V)[W])
{
    // bit j of vm[j >> 5]: column 64 h + j is a column of this lane
    const uint32_t left = lt > 64u * h ? lt - 64u * h : 0u;
    const uint32_t vm[2] = {low_ones(left), low_ones(left > 32u ? left - 32u : 0u)};
    unrolled_until<0, 64>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const uint32_t col = 64u * h + (uint32_t)j;
        if (col >= tmax) return false;
        const uint32_t valid = MASKED ? bit_fill(vm[j >> 5], j & 31) : 0xFFFFFFFFu;
        uint32_t Eq[W];
#pragma unroll
        for (int w = 0; w < W; ++w) Eq[w] = eq_mask<7>(P[w], valid, wt[j >> 2], j & 3);
        indel_lane_step<W>(Eq, V);
        return true;
    });
}

// l = the zero bits of V among the lp pattern rows
template <int W>
STRSIM_HD uint32_t indel_lane_lcs(const uint32_t (&V)[W], uint32_t lp)
{
    uint32_t l = 0u;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t r = lp > 32u * w ? lp - 32u * w : 0u;
        l += popc32(~V[w] & low_ones(r));
    }
    return l;
}

// One column of one 64-bit word of k_indel_wave; c is the carry in and out.
STRSIM_HD void indel_word_step(uint64_t Eq, uint64_t &V, uint64_t &c)
{
    const uint64_t u = V & Eq;
    const uint64_t s1 = V + u;
    const uint64_t s2 = s1 + c;
    c = (uint64_t)(s1 < u) | (uint64_t)(s2 < s1);
    V = s2 | (V & ~Eq);
}

// the LCS part of a word: zero bits of V among the rows of pattern word w (m rows in all)
STRSIM_HD uint32_t indel_word_lcs(uint64_t V, uint32_t w, uint32_t m)
{
    const uint32_t r = m - 64u * w;
    const uint64_t rows = r >= 64u ? ~0ull : ((1ull << r) - 1ull);
    return osa_popc((uint64_t)(~V & rows));
}

// k_indel_wave scratch of one wave for patterns of up to m scalar values: the values (padded to whole words of 64) and one 64-bit
// V per word.
STRSIM_HD uint64_t indel_wave_slot_words(uint64_t m)
{
    const uint64_t words = (m + 63u) / 64u;
    return words * 64u + words * 2u;
}

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

// max over the wave of v <= 255 by a binary search with ballots: eight compares, the result in a scalar register
__device__ __forceinline__ uint32_t indel_wave_max(uint32_t v)
{
    uint32_t g = 0u;
#pragma unroll
    for (uint32_t half = 128u; half >= 1u; half >>= 1)
        if (__ballot(v >= g + half) != 0ull) g += half;
    return g;
}

// The lane DP at one width: planes of the pattern's W windows, then the text in halves of 64 bytes (`halves` of them, wave-uniform).
// `hi` collects the high bits of every byte loaded (the ASCII test is made at the end: eq_mask compares seven bits, so a non-ASCII
// lane computes something harmless).  nt: the text bytes to load; lt_run: the columns of this lane (0 for a lane that runs none).
// UNI: the text is the same in every lane (a literal; tv, to and nt are wave-uniform), and its dwords are made scalar values, so
// that the seven bit fills of a column are scalar instructions and the vector unit is left the plane operations alone.
template <int W, bool UNI>
__device__ __forceinline__ uint32_t indel_lane_run(const uint8_t *__restrict__ pv, uint32_t po, uint32_t lp,
                                                   const uint8_t *__restrict__ tv, uint32_t to, uint32_t nt, uint32_t lt_run,
                                                   uint32_t tmax, uint32_t halves, uint32_t &hi)
{
    uint32_t P[W][7];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        uint32_t win[8];
        if (lp > 32u * w) {
            load_window32(pv, po + 32u * w, po + lp, win);
        } else {
#pragma unroll
            for (int d = 0; d < 8; ++d) win[d] = 0u;
        }
#pragma unroll
        for (int d = 0; d < 8; ++d) hi |= win[d];
        build_planes<7>(win, P[w]);
    }
    uint32_t V[W];
#pragma unroll
    for (int w = 0; w < W; ++w) V[w] = 0xFFFFFFFFu;
#pragma unroll 1
    for (uint32_t h = 0u; h < halves; ++h) {
        uint32_t wt[16];
        if (nt > 64u * h) {
            osa_load64(tv, to + 64u * h, nt - 64u * h < 64u ? nt - 64u * h : 64u, wt);
        } else {
#pragma unroll
            for (int d = 0; d < 16; ++d) wt[d] = 0u;
        }
        if constexpr (UNI) {
#pragma unroll
            for (int d = 0; d < 16; ++d) wt[d] = wave_uniform(wt[d]);
        }
#pragma unroll
        for (int d = 0; d < 16; ++d) hi |= wt[d];
        indel_lane_half<W, !UNI>(wt, h, lt_run, tmax, P, V);
    }
    return indel_lane_lcs<W>(V, lp);
}

// One pair per lane.  LIT as k_dist_lane: 0 = row against row (the longer string is the pattern), 1 = a is a literal, 2 = b is (the
// literal is the text, read through a wave-uniform address; the row is the pattern).  k: the distance cutoff (DIST_UNBOUNDED for
// the similarity); a pair of ASCII strings whose lengths differ by more than k is k + 1 without any column.  Rows this kernel
// cannot take are appended to `worklist` (worklist_append of strsim_wave_util.h); the status block is zeroed before the launch.
// (k_common_lcs_lane of strsim_common.h is this kernel under another epilogue: a change of the tier selection here belongs there too.)
template <int LIT>
__global__ __launch_bounds__(256) void k_indel_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA,
                                                    const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t n,
                                                    uint32_t k, double *__restrict__ out64, uint32_t *__restrict__ out32,
                                                    uint32_t *__restrict__ worklist, DevStatus *st)
{
    constexpr bool UNI = LIT != 0;
    const LaneRow r = lane_row(offA, offB, n, LIT == 1, LIT == 2);
    const uint64_t row = r.row;
    const uint32_t la = r.la, lb = r.lb;
    const bool live = r.live, fits = live && la <= INDEL_LANE_MAX_BYTES && lb <= INDEL_LANE_MAX_BYTES;
    const LanePick p = lane_pick<LIT>(valA, valB, r);
    const uint8_t *pv = p.pv, *tv = p.tv;
    const uint32_t po = p.po;
    // a lane that does not fit loads nothing and runs no column
    const uint32_t lp = fits ? p.lp : 0u, lt = fits ? p.lt : 0u;
    const bool cut = dist_length_cut(la, lb, k); // (holds for an ASCII row: bytes are scalar values)
    const uint32_t lt_run = cut ? 0u : lt;
    // The text as it is loaded: a literal by every lane alike (whether or not the lane's row fits), a row's by its lane.
    uint32_t to = p.to, nt = lt;
    if constexpr (UNI) {
        const uint32_t llit = wave_uniform(p.lt);
        to = wave_uniform(to);
        nt = llit <= INDEL_LANE_MAX_BYTES ? llit : 0u;
    }
    // wave-uniform, in scalar registers: the mask words of the wave, its columns, and the text halves it looks at (every fitting
    // row is tested for ASCII, also one that runs no column)
    const uint32_t words = 1u + (__ballot(lp > 32u) != 0ull) + (__ballot(lp > 64u) != 0ull) + (__ballot(lp > 96u) != 0ull);
    const uint32_t tmax = UNI ? (__ballot(lt_run != 0u) != 0ull ? nt : 0u) : indel_wave_max(lt_run);
    const uint32_t halves = UNI ? (nt > 64u ? 2u : 1u) : (__ballot(lt > 64u) != 0ull ? 2u : 1u);
    uint32_t hi = 0u, l = 0u;
    if (words == 1u) l = indel_lane_run<1, UNI>(pv, po, lp, tv, to, nt, lt_run, tmax, halves, hi);
    else if (words == 2u) l = indel_lane_run<2, UNI>(pv, po, lp, tv, to, nt, lt_run, tmax, halves, hi);
    else if (words == 3u) l = indel_lane_run<3, UNI>(pv, po, lp, tv, to, nt, lt_run, tmax, halves, hi);
    else l = indel_lane_run<4, UNI>(pv, po, lp, tv, to, nt, lt_run, tmax, halves, hi);
    const bool ok = fits && (hi & 0x80808080u) == 0u;
    worklist_append<false>(live && !ok, row, la, lb, worklist, st); // rows for k_indel_wave
    if (ok) {
        const uint32_t d = la + lb - 2u * l;
        if (out32) out32[row] = cut ? k + 1u : dist_clamp(d, k);
        else out64[row] = epilogue_indel(d, la, lb);
    }
}

// The columns of one pair with the pattern (m <= 64 NW values, decoded into pat and padded to 64 NW) in registers: pv[w] is this
// lane's value of word w, V is wave-uniform.  Nothing goes through memory in the column loop.
template <int NW>
__device__ __forceinline__ uint32_t indel_wave_reg(const uint32_t *pat, uint32_t m, const uint8_t *__restrict__ tp, uint32_t tbytes,
                                                   uint32_t lane)
{
    uint32_t pv[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) pv[w] = pat[64 * w + lane];
    uint64_t V[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) V[w] = ~0ull;
    wave_each_char(tp, tbytes, lane, [&](uint32_t ch) {
        uint64_t c = 0ull;
#pragma unroll
        for (int w = 0; w < NW; ++w) indel_word_step((uint64_t)__ballot(pv[w] == ch), V[w], c);
    });
    uint32_t l = 0u;
#pragma unroll
    for (int w = 0; w < NW; ++w)
        if (m > 64u * w) l += indel_word_lcs(V[w], (uint32_t)w, m);
    return l;
}

// One pair per wave (blockDim.x = 64) for the rows k_indel_lane put on the work list (st->wave_rows of them).  The shorter string
// (in scalar values) is the pattern.  scratch: gridDim.x slots of slot_words words, for patterns of more than OSA_WAVE_LDS_CPS
// values (nullptr when the call has none).
// (k_common_lcs_wave of strsim_common.h is this kernel under another epilogue: a change of the forms here belongs there too.)
__global__ __launch_bounds__(64) void k_indel_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                   const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                                   uint32_t k, double *__restrict__ out64, uint32_t *__restrict__ out32,
                                                   const uint32_t *__restrict__ worklist, const DevStatus *st, uint32_t *scratch,
                                                   uint64_t slot_words)
{
    __shared__ uint32_t s_pat[OSA_WAVE_LDS_CPS];
    __shared__ uint64_t s_state[OSA_WAVE_LDS_CPS / 64u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = st->wave_rows;
    for (uint32_t r = blockIdx.x; r < count; r += gridDim.x) {
        const WavePair p = wave_pair(offA, valA, rowsA, offB, valB, rowsB, worklist[r]);
        const WaveStage<uint64_t> s = wave_stage(p, s_pat, s_state, OSA_WAVE_LDS_CPS, scratch, slot_words);
        const uint32_t row = p.row, ca = p.ca, cb = p.cb, m = s.m, W = s.W, tbytes = s.tbytes;
        const uint8_t *tp = s.tp;
        uint32_t *const pat = s.pat;
        uint64_t *const state = s.state;
        const bool cut = dist_length_cut(ca, cb, k);
        uint32_t l = 0u;
        if (!cut && m != 0u) {
            wave_pattern(s.pp, s.pbytes, m, W == 3u ? 4u : W, pat, lane); // (the register form has 1, 2 or 4 words)
            for (uint32_t w = lane; w < W; w += 64u) state[w] = ~0ull;
            __syncthreads();
            if (W == 1u) l = indel_wave_reg<1>(pat, m, tp, tbytes, lane);
            else if (W == 2u) l = indel_wave_reg<2>(pat, m, tp, tbytes, lane);
            else if (64u * W <= INDEL_WAVE_REG_CPS) l = indel_wave_reg<4>(pat, m, tp, tbytes, lane);
            else {
                wave_each_char(tp, tbytes, lane, [&](uint32_t ch) {
                    uint64_t c = 0ull;
                    for (uint32_t w = 0; w < W; ++w) {
                        uint64_t V = state[w];
                        indel_word_step((uint64_t)__ballot(pat[64u * w + lane] == ch), V, c);
                        state[w] = V;
                    }
                });
                for (uint32_t w = 0; w < W; ++w) l += indel_word_lcs(state[w], w, m);
            }
            __syncthreads(); // (the next row overwrites pat / state)
        }
        if (lane == 0u) {
            const uint64_t d = (uint64_t)ca + cb - 2ull * l;
            if (out32) out32[row] = cut ? k + 1u : dist_clamp(d, k);
            else out64[row] = epilogue_indel(d, ca, cb);
        }
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
