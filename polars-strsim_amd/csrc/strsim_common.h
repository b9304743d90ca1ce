// strsim_common.h -- Hamming, prefix, postfix and LCSseq similarity, distance and count (strsim_common_device / _host,
// strsim_common_distance_device / _host, strsim_common_count_device / _host).  They have no measure id.
//
// Each kind is a count c(a, b) of what the two strings share, over Unicode scalar values, at most min(|a|, |b|):
//   COMMON_HAMMING  positions i < min(|a|, |b|) with a_i == b_i
//   COMMON_PREFIX   length of the longest common prefix
//   COMMON_POSTFIX  length of the longest common suffix
//   COMMON_LCSSEQ   length of the longest common subsequence
// and the three outputs follow from it as in rapidfuzz.distance.{Hamming, Prefix, Postfix, LCSseq}: the count itself, the distance
// d = max(|a|, |b|) - c (for Hamming: mismatches plus the difference of the lengths, rapidfuzz's pad=True) written as d when
// d <= k and k + 1 otherwise (dist_clamp), and the similarity epilogue_osa(d, |a|, |b|) = 1 - d / max(|a|, |b|), 1.0 when both are
// empty.  d >= | |a| - |b| | for all four, so the length prefilter of the distances (dist_length_cut) holds here too.
//
// The three positional kinds, both tiers finished in stream order:
//   k_common_lane<KIND, LIT, OUT>  one pair per lane, both strings ASCII and <= COMMON_LANE_MAX bytes.  The two 32-byte windows
//                        are XORed dword by dword and the non-zero bytes gathered into one 32-bit mask (common_diff_mask): Hamming is
//                        a popcount of its complement, prefix a count of trailing zeros, postfix a count of leading zeros after the
//                        longer window was moved down by | |a| - |b| | bytes so that the ends line up (common_shift_down: a
//                        logarithmic shifter of selects between registers with constant indices, then v_alignbyte_b32 -- no
//                        register is ever indexed by a lane's value).  Every other row is appended to the work list.
//   k_common_wave<KIND, OUT>  one pair per wave for the work list: any UTF-8, any length, streamed 64 bytes at a time.  It keeps no
//                        copy of a string and uses none of the context's scratch.
//     Prefix and postfix stay at byte level.  Both strings are valid UTF-8, where a lead byte fixes the width of its character
//     and no lead byte is a continuation byte.  With p the length of the common byte prefix: a character of a that starts in
//     a[0, p) has its lead byte in common with b, hence b has a character of the same width at the same place; it is a common
//     character iff all its bytes lie in front of p.  Only the last start can fail that, and it does exactly when a[p] exists
//     and is a continuation byte: c = starts in a[0, p), minus one in that case (common_prefix_chunk).  With s the length of the
//     common byte suffix: a character whose lead byte lies in the suffix lies in it whole (the suffix runs to the end) and b has the
//     same lead byte, hence the same character, there; one whose lead byte lies in front of it differs from b's or is cut by it.
//     c = starts inside the suffix (common_suffix_chunk).
//     Hamming compares the two character streams in lockstep although their byte positions drift: each string has a byte cursor of
//     its own; a step looks at 64 bytes behind each cursor, ballots the character starts and ranks them, takes t = the smaller of
//     the two counts, has the lane that holds the k-th start (k < t) decode it into slot k of a 64-entry LDS stage per string,
//     compares the slots, and moves each cursor to its t-th start (common_lockstep).  A pair of ASCII strings (too long for the lane
//     tier) skips the decode and compares bytes.
// LCSseq is not a new DP: k_common_lcs_lane / k_common_lcs_wave run the bit-parallel step of strsim_indel.h (indel_lane_run, its
// planes and text walk; indel_wave_reg and the word step) with Indel's classes and scratch, under this header's epilogue, with
// c = popc(~V & rows).
//
// OUT: COMMON_OUT_SIM the f64 similarity, COMMON_OUT_DIST the uint32 distance under the cutoff, COMMON_OUT_COUNT the uint32 count.
#pragma once
#include <stdint.h>

#include "strsim_bounds.h"
#include "strsim_distance.h"
#include "strsim_indel.h"

namespace strsim {

enum CommonKind : int { COMMON_HAMMING = 0, COMMON_PREFIX = 1, COMMON_POSTFIX = 2, COMMON_LCSSEQ = 3 }; // = STRSIM_COMMON_*
enum CommonOut : int { COMMON_OUT_SIM = 0, COMMON_OUT_DIST = 1, COMMON_OUT_COUNT = 2 };

constexpr uint32_t COMMON_LANE_MAX = 32u; // k_common_lane: both strings ASCII and at most this long (one load_window32 each)

STRSIM_HD uint32_t common_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
STRSIM_HD uint32_t common_max(uint32_t a, uint32_t b) { return a < b ? b : a; }
STRSIM_HD uint64_t common_low_ones64(uint32_t k) { return k >= 64u ? ~0ull : ((1ull << k) - 1ull); }

// the distance of a pair with c in common (la, lb: scalar values)
STRSIM_HD uint64_t common_distance(uint64_t c, uint64_t la, uint64_t lb) { return (la > lb ? la : lb) - c; }

// ---- the lane core: 32-byte windows of ASCII bytes, zero past the end of the string ----

// bit i: byte i of the two windows differs.  Every byte of x is < 0x80, so adding 0x7F sets bit 7 of exactly the non-zero bytes and
// nothing is carried from one byte into the next; the multiplication gathers the four flags (bits 0, 8, 16, 24) in bits 24..27.
STRSIM_HD uint32_t common_diff_mask(const uint32_t (&wa)[8], const uint32_t (&wb)[8])
{
    uint32_t n = 0u;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const uint32_t x = wa[d] ^ wb[d];
        const uint32_t nz = ((x + 0x7F7F7F7Fu) >> 7) & 0x01010101u;
        n |= ((nz * 0x01020408u) >> 24) << (4 * d);
    }
    return n;
}

// the byte-window count per kind, from the mask of differing bytes and m = min(la, lb) <= 32
STRSIM_HD uint32_t common_hamming32(uint32_t diff, uint32_t m) { return popc32(~diff & low_ones(m)); }
STRSIM_HD uint32_t common_prefix32(uint32_t diff, uint32_t m)
{
    const uint32_t x = diff | ~low_ones(m); // (byte m ends the prefix at the latest)
    return x ? (uint32_t)__builtin_ctz(x) : 32u;
}
STRSIM_HD uint32_t common_suffix32(uint32_t diff, uint32_t m)
{
    const uint32_t y = diff & low_ones(m); // bytes m - 1 downward are the suffix
    return y ? m - 32u + (uint32_t)__builtin_clz(y) : m;
}

// ({hi, lo} >> 8 r) & 0xFFFFFFFF, r = 0..3: v_alignbyte_b32
STRSIM_HD uint32_t common_alignbyte(uint32_t hi, uint32_t lo, uint32_t r)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * (r & 3u)));
#endif
}

// The end alignment: the window moved down by delta bytes (0..32), w'[i] = w[i + delta], zero shifted in.  Whole dwords by a
// logarithmic shifter -- per stage every register takes itself or the one 8, 4, 2 or 1 above it, a select between two registers
// with constant indices --, the last 0..3 bytes by a funnel shift across neighbouring dwords.
STRSIM_HD void common_shift_down(uint32_t (&w)[8], uint32_t delta)
{
    const uint32_t q = delta >> 2, r = delta & 3u;
#pragma unroll
    for (int d = 0; d < 8; ++d) w[d] = (q & 8u) ? 0u : w[d];
#pragma unroll
    for (int d = 0; d < 8; ++d) w[d] = (q & 4u) ? (d + 4 < 8 ? w[d + 4 < 8 ? d + 4 : 7] : 0u) : w[d];
#pragma unroll
    for (int d = 0; d < 8; ++d) w[d] = (q & 2u) ? (d + 2 < 8 ? w[d + 2 < 8 ? d + 2 : 7] : 0u) : w[d];
#pragma unroll
    for (int d = 0; d < 8; ++d) w[d] = (q & 1u) ? (d + 1 < 8 ? w[d + 1 < 8 ? d + 1 : 7] : 0u) : w[d];
#pragma unroll
    for (int d = 0; d < 8; ++d) w[d] = common_alignbyte(d + 1 < 8 ? w[d + 1 < 8 ? d + 1 : 7] : 0u, w[d], r);
}

// c of a pair of ASCII strings of la, lb <= COMMON_LANE_MAX bytes in the windows wa, wb (all three kinds are symmetric)
template <int KIND>
STRSIM_HD uint32_t common_lane_count(const uint32_t (&wa)[8], uint32_t la, const uint32_t (&wb)[8], uint32_t lb)
{
    const uint32_t m = common_min(la, lb);
    if constexpr (KIND == COMMON_POSTFIX) {
        const bool a_long = la >= lb;
        uint32_t wl[8], ws[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            wl[d] = a_long ? wa[d] : wb[d];
            ws[d] = a_long ? wb[d] : wa[d];
        }
        common_shift_down(wl, common_max(la, lb) - m);
        return common_suffix32(common_diff_mask(wl, ws), m);
    } else if constexpr (KIND == COMMON_PREFIX) {
        return common_prefix32(common_diff_mask(wa, wb), m);
    } else {
        return common_hamming32(common_diff_mask(wa, wb), m);
    }
}

// What k_common_lane does with a row (DistRow of strsim_distance.h); ascii is only looked at for a row that fits.
STRSIM_HD bool common_lane_fits(uint32_t la, uint32_t lb) { return la <= COMMON_LANE_MAX && lb <= COMMON_LANE_MAX; }
STRSIM_HD uint32_t common_lane_row(bool live, uint32_t la, uint32_t lb, bool ascii, uint32_t k)
{
    if (!live) return DIST_ROW_NONE;
    if (!common_lane_fits(la, lb) || !ascii) return DIST_ROW_WAVE;
    return dist_length_cut(la, lb, k) ? DIST_ROW_CUT : DIST_ROW_RUN;
}

// ---- the wave core: 64 byte positions at a time, as masks with one bit a lane ----

// One chunk of the byte prefix walk.  mm: the two strings differ at the position, or one of them has ended there; sa / ka: a has a
// character start / a continuation byte there.  Adds the chunk's common characters to c; true: the prefix ends in this chunk.
STRSIM_HD bool common_prefix_chunk(uint64_t mm, uint64_t sa, uint64_t ka, uint32_t &c)
{
    if (mm == 0ull) {
        c += osa_popc(sa);
        return false;
    }
    const uint32_t f = (uint32_t)__builtin_ctzll(mm);
    c += osa_popc((uint64_t)(sa & common_low_ones64(f)));
    if (((ka >> f) & 1ull) != 0ull && c != 0u) c -= 1u; // a[p] continues the last character that started: it is cut
    return true;
}

// One chunk of the byte suffix walk, bit i the position i bytes in front of the chunk's last.  Arguments as above.
STRSIM_HD bool common_suffix_chunk(uint64_t mm, uint64_t sa, uint32_t &c)
{
    if (mm == 0ull) {
        c += osa_popc(sa);
        return false;
    }
    c += osa_popc((uint64_t)(sa & common_low_ones64((uint32_t)__builtin_ctzll(mm))));
    return true;
}

// the position of set bit number t (from 0) of mask; t < popcount(mask)
STRSIM_HD uint32_t common_nth_set(uint64_t mask, uint32_t t)
{
    uint32_t pos = 0u;
#pragma unroll
    for (uint32_t w = 32u; w >= 1u; w >>= 1) {
        const uint32_t cnt = osa_popc((uint64_t)((mask >> pos) & common_low_ones64(w)));
        if (cnt <= t) {
            t -= cnt;
            pos += w;
        }
    }
    return pos;
}

// One step of the lockstep walk.  ma / mb: the character starts among the 64 bytes behind each string's cursor.  t characters of
// each are compared, and each cursor moves to its start number t, or past the chunk when it has no more than t.
struct CommonStep {
    uint32_t t, adva, advb;
};
STRSIM_HD CommonStep common_lockstep(uint64_t ma, uint64_t mb)
{
    const uint32_t sa = osa_popc(ma), sb = osa_popc(mb);
    CommonStep s;
    s.t = common_min(sa, sb);
    s.adva = s.t < sa ? common_nth_set(ma, s.t) : 64u;
    s.advb = s.t < sb ? common_nth_set(mb, s.t) : 64u;
    return s;
}

// a cursor moved on by adv, never past the end of its string (which keeps cursor + lane below 2^32)
STRSIM_HD uint32_t common_advance(uint32_t cur, uint32_t adv, uint32_t len) { return len - cur < adv ? len : cur + adv; }

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

// what both tiers write for a pair of la and lb scalar values with c in common
template <int OUT>
__device__ __forceinline__ void common_store(void *out, uint64_t row, uint64_t c, uint64_t la, uint64_t lb, uint32_t k)
{
    const uint64_t d = common_distance(c, la, lb);
    if constexpr (OUT == COMMON_OUT_SIM) static_cast<double *>(out)[row] = epilogue_osa(d, la, lb);
    else if constexpr (OUT == COMMON_OUT_DIST) static_cast<uint32_t *>(out)[row] = dist_clamp(d, k);
    else static_cast<uint32_t *>(out)[row] = (uint32_t)c;
}
// the same with the output chosen at run time (the LCSseq kernels)
__device__ __forceinline__ void common_store_as(int mode, void *out, uint64_t row, uint64_t c, uint64_t la, uint64_t lb, uint32_t k)
{
    if (mode == COMMON_OUT_SIM) common_store<COMMON_OUT_SIM>(out, row, c, la, lb, k);
    else if (mode == COMMON_OUT_DIST) common_store<COMMON_OUT_DIST>(out, row, c, la, lb, k);
    else common_store<COMMON_OUT_COUNT>(out, row, c, la, lb, k);
}

// One pair per lane.  LIT as k_dist_lane: a literal is read through a wave-uniform address.  OUT = COMMON_OUT_DIST: the distance
// under the cutoff kcut, a row whose lengths differ by more than it is kcut + 1 at once; the other outputs do not look at kcut.
// Rows this kernel cannot take are appended to `worklist`; st->wave_rows counts them.  The status block is zeroed before the launch.
template <int KIND, int LIT, int OUT>
__global__ __launch_bounds__(256) void k_common_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA,
                                                     const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t n,
                                                     uint32_t kcut, void *__restrict__ out, uint32_t *__restrict__ worklist, DevStatus *st)
{
    const uint32_t k = OUT == COMMON_OUT_DIST ? kcut : DIST_UNBOUNDED;
    const LaneRow r = lane_row(offA, offB, n, LIT == 1, LIT == 2);
    const uint32_t la = r.la, lb = r.lb;
    const bool fits = r.live && common_lane_fits(la, lb);
    const LanePick p = lane_pick<LIT>(valA, valB, r);
    uint32_t wp[8] = {}, wt[8] = {};
    bool ascii = false;
    if (fits) {
        STRSIM_CHECK_RANGE(K_COMMON, 1, r.row, p.lp, 0, COMMON_LANE_MAX);
        STRSIM_CHECK_RANGE(K_COMMON, 2, r.row, p.lt, 0, COMMON_LANE_MAX);
        load_window32(p.pv, p.po, p.po + p.lp, wp);
        load_window32(p.tv, p.to, p.to + p.lt, wt);
        uint32_t o = 0u;
#pragma unroll
        for (int d = 0; d < 8; ++d) o |= wp[d] | wt[d];
        ascii = (o & 0x80808080u) == 0u;
    }
    const uint32_t cls = common_lane_row(r.live, la, lb, ascii, k);
    worklist_append<false>(cls == DIST_ROW_WAVE, r.row, la, lb, worklist, st); // rows for k_common_wave
    if constexpr (OUT == COMMON_OUT_DIST)
        if (cls == DIST_ROW_CUT) static_cast<uint32_t *>(out)[r.row] = k + 1u;
    if (cls == DIST_ROW_RUN) {
        const uint32_t c = common_lane_count<KIND>(wp, p.lp, wt, p.lt);
        STRSIM_CHECK_RANGE(K_COMMON, 3, r.row, c, 0, common_min(la, lb));
        common_store<OUT>(out, r.row, c, la, lb, k);
    }
}

// The common byte prefix of a[0, na) and b[0, nb) in characters, by the wave.
__device__ __forceinline__ uint32_t common_wave_prefix(const uint8_t *__restrict__ a, uint32_t na, const uint8_t *__restrict__ b, uint32_t nb,
                                                       uint32_t lane, uint32_t row)
{
    const uint32_t m = common_min(na, nb); // (the walk ends in the chunk that holds position m; only the lab build looks at it)
    (void)m;
    uint32_t c = 0u;
    // (the chunk that holds position m ends the walk: a string that has ended differs from everything)
    for (uint32_t base = 0u;; base += 64u) {
        STRSIM_CHECK_RANGE(K_COMMON, 10, row, base, 0, m);
        const uint32_t i = base + lane; // (base <= m and lane < 64: below 2^32 + 63 only for m near 2^32, which the clamp below covers)
        const bool ina = i >= base && i < na, inb = i >= base && i < nb;
        if (ina) STRSIM_CHECK_INDEX(K_COMMON, 12, row, i, na);
        if (inb) STRSIM_CHECK_INDEX(K_COMMON, 13, row, i, nb);
        const uint32_t xa = ina ? (uint32_t)a[i] : 0x100u, xb = inb ? (uint32_t)b[i] : 0x200u;
        const uint64_t mm = __ballot(xa != xb);
        const uint64_t sa = __ballot(ina && (xa & 0xC0u) != 0x80u), ka = __ballot(ina && (xa & 0xC0u) == 0x80u);
        if (common_prefix_chunk(mm, sa, ka, c)) break;
    }
    return c;
}

// The common byte suffix in characters; position i of the walk is byte len - 1 - i of each string, never one in front of it.
__device__ __forceinline__ uint32_t common_wave_suffix(const uint8_t *__restrict__ a, uint32_t na, const uint8_t *__restrict__ b, uint32_t nb,
                                                       uint32_t lane, uint32_t row)
{
    const uint32_t m = common_min(na, nb); // (the walk ends in the chunk that holds position m; only the lab build looks at it)
    (void)m;
    uint32_t c = 0u;
    for (uint32_t base = 0u;; base += 64u) {
        STRSIM_CHECK_RANGE(K_COMMON, 11, row, base, 0, m);
        const uint32_t i = base + lane;
        const bool ina = i >= base && i < na, inb = i >= base && i < nb;
        if (ina) STRSIM_CHECK_INDEX(K_COMMON, 14, row, na - 1u - i, na);
        if (inb) STRSIM_CHECK_INDEX(K_COMMON, 15, row, nb - 1u - i, nb);
        const uint32_t xa = ina ? (uint32_t)a[na - 1u - i] : 0x100u, xb = inb ? (uint32_t)b[nb - 1u - i] : 0x200u;
        const uint64_t mm = __ballot(xa != xb);
        const uint64_t sa = __ballot(ina && (xa & 0xC0u) != 0x80u);
        if (common_suffix_chunk(mm, sa, c)) break;
    }
    return c;
}

// Equal positions of two ASCII strings (bytes are characters).
__device__ __forceinline__ uint32_t common_wave_hamming_bytes(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t m,
                                                              uint32_t lane, uint32_t row)
{
    uint32_t c = 0u;
    for (uint32_t base = 0u; base < m; base += 64u) {
        const uint32_t i = base + lane;
        const bool in = i >= base && i < m;
        const uint32_t at = in ? i : 0u; // (m >= 1 here: position 0 exists in both strings)
        STRSIM_CHECK_INDEX(K_COMMON, 16, row, at, m);
        c += (uint32_t)__popcll(__ballot(in && a[at] == b[at]));
    }
    return c;
}

// Equal positions of the two character streams (the lockstep walk of the header comment).  s_a / s_b: 64 words each.
__device__ __forceinline__ uint32_t common_wave_hamming(const uint8_t *__restrict__ a, uint32_t na, const uint8_t *__restrict__ b, uint32_t nb,
                                                        uint32_t *s_a, uint32_t *s_b, uint32_t lane, uint32_t row)
{
    uint32_t cura = 0u, curb = 0u, c = 0u;
    for (;;) {
        STRSIM_CHECK_RANGE(K_COMMON, 20, row, cura, 0, na);
        STRSIM_CHECK_RANGE(K_COMMON, 21, row, curb, 0, nb);
        // (a cursor is at most len and stops there, so cursor + lane wraps only beside a string of nearly 2^32 bytes: i >= cur)
        const uint32_t ia = cura + lane, ib = curb + lane;
        if (ia >= cura && ia < na) STRSIM_CHECK_INDEX(K_COMMON, 24, row, ia, na);
        if (ib >= curb && ib < nb) STRSIM_CHECK_INDEX(K_COMMON, 25, row, ib, nb);
        const bool sta = ia >= cura && osa_is_start(a, ia, na), stb = ib >= curb && osa_is_start(b, ib, nb);
        const uint64_t ma = __ballot(sta), mb = __ballot(stb);
        const CommonStep s = common_lockstep(ma, mb);
        if (s.t == 0u && (cura >= na || curb >= nb)) break; // one string has no character left
        if (s.t != 0u) {
            const uint32_t ra = (uint32_t)__popcll(ma & ((1ull << lane) - 1ull)), rb = (uint32_t)__popcll(mb & ((1ull << lane) - 1ull));
            if (sta && ra < s.t) {
                STRSIM_CHECK_INDEX(K_COMMON, 22, row, ra, 64);
                s_a[ra] = osa_decode_at(a, ia, na);
            }
            if (stb && rb < s.t) {
                STRSIM_CHECK_INDEX(K_COMMON, 23, row, rb, 64);
                s_b[rb] = osa_decode_at(b, ib, nb);
            }
            __syncthreads();
            c += (uint32_t)__popcll(__ballot(lane < s.t && s_a[lane] == s_b[lane]));
            __syncthreads(); // (the next step overwrites the stages)
        }
        // (without a start among 64 bytes in range -- not UTF-8 -- that string alone moves on)
        cura = common_advance(cura, s.t == 0u && ma != 0ull ? 0u : s.adva, na);
        curb = common_advance(curb, s.t == 0u && mb != 0ull ? 0u : s.advb, nb);
    }
    return c;
}

// One pair per wave (blockDim.x = 64) for the rows k_common_lane put on the work list (st->wave_rows of them).  OUT as k_common_lane.
template <int KIND, int OUT>
__global__ __launch_bounds__(64) void k_common_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                    const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                                    uint32_t kcut, void *__restrict__ out, const uint32_t *__restrict__ worklist,
                                                    const DevStatus *st)
{
    const uint32_t k = OUT == COMMON_OUT_DIST ? kcut : DIST_UNBOUNDED;
    __shared__ uint32_t s_a[64], s_b[64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = st->wave_rows;
    for (uint32_t r = blockIdx.x; r < count; r += gridDim.x) {
        STRSIM_CHECK_INDEX(K_COMMON, 30, r, worklist[r], rowsA > rowsB ? rowsA : rowsB);
        const WavePair p = wave_pair(offA, valA, rowsA, offB, valB, rowsB, worklist[r]);
        const bool cut = dist_length_cut(p.ca, p.cb, k);
        uint32_t c = 0u;
        if (!cut) {
            if constexpr (KIND == COMMON_PREFIX) c = common_wave_prefix(p.pa, p.na, p.pb, p.nb, lane, p.row);
            else if constexpr (KIND == COMMON_POSTFIX) c = common_wave_suffix(p.pa, p.na, p.pb, p.nb, lane, p.row);
            else if (p.ca == p.na && p.cb == p.nb) c = common_wave_hamming_bytes(p.pa, p.pb, common_min(p.na, p.nb), lane, p.row);
            else c = common_wave_hamming(p.pa, p.na, p.pb, p.nb, s_a, s_b, lane, p.row);
            STRSIM_CHECK_RANGE(K_COMMON, 31, p.row, c, 0, common_min(p.ca, p.cb));
        }
        if (lane == 0u) {
            if (OUT == COMMON_OUT_DIST && cut) static_cast<uint32_t *>(out)[p.row] = k + 1u;
            else common_store<OUT>(out, p.row, c, p.ca, p.cb, k);
        }
    }
}

// LCSseq, one pair per lane: k_indel_lane's set-up and its indel_lane_run, Indel's class (ASCII, <= INDEL_LANE_MAX_BYTES), the
// epilogue of this header.  mode: a CommonOut; k is DIST_UNBOUNDED unless mode is COMMON_OUT_DIST.
template <int LIT>
__global__ __launch_bounds__(256) void k_common_lcs_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA,
                                                         const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t n,
                                                         uint32_t k, int mode, void *__restrict__ out, uint32_t *__restrict__ worklist,
                                                         DevStatus *st)
{
    constexpr bool UNI = LIT != 0;
    const LaneRow r = lane_row(offA, offB, n, LIT == 1, LIT == 2);
    const uint64_t row = r.row;
    const uint32_t la = r.la, lb = r.lb;
    const bool live = r.live, fits = live && la <= INDEL_LANE_MAX_BYTES && lb <= INDEL_LANE_MAX_BYTES;
    const LanePick p = lane_pick<LIT>(valA, valB, r);
    const uint32_t lp = fits ? p.lp : 0u, lt = fits ? p.lt : 0u;
    const bool cut = dist_length_cut(la, lb, k);
    const uint32_t lt_run = cut ? 0u : lt;
    uint32_t to = p.to, nt = lt;
    if constexpr (UNI) {
        const uint32_t llit = wave_uniform(p.lt);
        to = wave_uniform(to);
        nt = llit <= INDEL_LANE_MAX_BYTES ? llit : 0u;
    }
    const uint32_t words = 1u + (__ballot(lp > 32u) != 0ull) + (__ballot(lp > 64u) != 0ull) + (__ballot(lp > 96u) != 0ull);
    const uint32_t tmax = UNI ? (__ballot(lt_run != 0u) != 0ull ? nt : 0u) : indel_wave_max(lt_run);
    const uint32_t halves = UNI ? (nt > 64u ? 2u : 1u) : (__ballot(lt > 64u) != 0ull ? 2u : 1u);
    STRSIM_CHECK_RANGE(K_COMMON, 40, row, tmax, 0, INDEL_LANE_MAX_BYTES);
    uint32_t hi = 0u, l = 0u;
    if (words == 1u) l = indel_lane_run<1, UNI>(p.pv, p.po, lp, p.tv, to, nt, lt_run, tmax, halves, hi);
    else if (words == 2u) l = indel_lane_run<2, UNI>(p.pv, p.po, lp, p.tv, to, nt, lt_run, tmax, halves, hi);
    else if (words == 3u) l = indel_lane_run<3, UNI>(p.pv, p.po, lp, p.tv, to, nt, lt_run, tmax, halves, hi);
    else l = indel_lane_run<4, UNI>(p.pv, p.po, lp, p.tv, to, nt, lt_run, tmax, halves, hi);
    const bool ok = fits && (hi & 0x80808080u) == 0u;
    worklist_append<false>(live && !ok, row, la, lb, worklist, st); // rows for k_common_lcs_wave
    if (ok) {
        STRSIM_CHECK_RANGE(K_COMMON, 41, row, l, 0, common_min(la, lb));
        if (cut) static_cast<uint32_t *>(out)[row] = k + 1u; // (mode is COMMON_OUT_DIST)
        else common_store_as(mode, out, row, l, la, lb, k);
    }
}

// LCSseq, one pair per wave for the work list: k_indel_wave's staging, register and LDS forms and its scratch slot (patterns of more
// than OSA_WAVE_LDS_CPS values: indel_wave_slot_words), the epilogue of this header.
__global__ __launch_bounds__(64) void k_common_lcs_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                        const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                                        uint32_t k, int mode, void *__restrict__ out, const uint32_t *__restrict__ worklist,
                                                        const DevStatus *st, uint32_t *scratch, uint64_t slot_words)
{
    __shared__ uint32_t s_pat[OSA_WAVE_LDS_CPS];
    __shared__ uint64_t s_state[OSA_WAVE_LDS_CPS / 64u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = st->wave_rows;
    for (uint32_t r = blockIdx.x; r < count; r += gridDim.x) {
        STRSIM_CHECK_INDEX(K_COMMON, 50, r, worklist[r], rowsA > rowsB ? rowsA : rowsB);
        const WavePair p = wave_pair(offA, valA, rowsA, offB, valB, rowsB, worklist[r]);
        const WaveStage<uint64_t> s = wave_stage(p, s_pat, s_state, OSA_WAVE_LDS_CPS, scratch, slot_words);
        const uint32_t m = s.m, W = s.W;
        if (m > OSA_WAVE_LDS_CPS) STRSIM_CHECK_RANGE(K_COMMON, 51, p.row, indel_wave_slot_words(m), 0, slot_words);
        const bool cut = dist_length_cut(p.ca, p.cb, k);
        uint32_t l = 0u;
        if (!cut && m != 0u) {
            wave_pattern(s.pp, s.pbytes, m, W == 3u ? 4u : W, s.pat, lane); // (the register form has 1, 2 or 4 words)
            for (uint32_t w = lane; w < W; w += 64u) s.state[w] = ~0ull;
            __syncthreads();
            if (W == 1u) l = indel_wave_reg<1>(s.pat, m, s.tp, s.tbytes, lane);
            else if (W == 2u) l = indel_wave_reg<2>(s.pat, m, s.tp, s.tbytes, lane);
            else if (64u * W <= INDEL_WAVE_REG_CPS) l = indel_wave_reg<4>(s.pat, m, s.tp, s.tbytes, lane);
            else {
                wave_each_char(s.tp, s.tbytes, lane, [&](uint32_t ch) {
                    uint64_t c = 0ull;
                    for (uint32_t w = 0; w < W; ++w) {
                        uint64_t V = s.state[w];
                        indel_word_step((uint64_t)__ballot(s.pat[64u * w + lane] == ch), V, c);
                        s.state[w] = V;
                    }
                });
                for (uint32_t w = 0; w < W; ++w) l += indel_word_lcs(s.state[w], w, m);
            }
            __syncthreads(); // (the next row overwrites pat / state)
        }
        if (lane == 0u) {
            if (cut) static_cast<uint32_t *>(out)[p.row] = k + 1u; // (mode is COMMON_OUT_DIST)
            else common_store_as(mode, out, p.row, l, p.ca, p.cb, k);
        }
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
