// strsim_token.h -- token_sort_ratio and token_set_ratio (measure ids 14 and 16): tokenising, sorting tokens and set operations on
// strings in device memory.  The alignment itself is Indel's (strsim_indel.h), run over the columns this header writes.
//
// Whitespace is Python's str.isspace set (29 code points), tokens are the maximal runs of anything else (str.split()), token order is
// bytewise order of the UTF-8 (= lexicographic order of the scalar values, a proper prefix first), join puts one U+0020 between tokens.
//   sort form  a row becomes join(sorted(tokens)); never longer than the input.
//   set form   a pair becomes ab = join(sorted(A - B)), ba = join(sorted(B - A)) and a record {sl, la, lb, flags}: the lengths in
//              scalar values of join(sorted(A & B)), ab and ba, and which of the two early answers of the rule applies
//              (token_set_score).  A and B are the SETS of tokens.
//
// Every form runs twice: a measuring pass that leaves the output lengths (a device scan turns them into offsets), then a writing
// pass.  Two tiers:
//   k_token_*_lane  one string (set form: one pair) per lane: ASCII, at most TOKEN_LANE_MAX_BYTES bytes and TOKEN_LANE_MAX_TOKENS
//                   tokens a string.  Token descriptors (start, length: a byte each) in LDS as [slot][thread], insertion sort.
//                   Every other row is appended to a work list by the measuring pass.
//   k_token_*_wave  one string (pair) per wave for the work list: any UTF-8, every whitespace code point, any length, any token
//                   count.  The wave finds the token starts of 64 bytes at a time, sorts the descriptors with a bitonic network
//                   whose comparators all point the same way (so that no padding is stored), then walks the sorted lists with every
//                   lane on the same token and copies its bytes 64 at a time.  Descriptors live in LDS up to TOKEN_WAVE_LDS_TOKENS
//                   of them and in a slot of the context's scratch above that.  Correct, not tuned.
// The cores below (whitespace test, token bounds, comparison, sorts, join, merge, score) are host/device code:
// tests/cpu_harness/token_harness.cpp compiles them with g++.
#pragma once
#include <stdint.h>

#include "strsim_indel.h"

namespace strsim {

constexpr int TOKEN_SORT_RATIO = 14;               // = STRSIM_TOKEN_SORT_RATIO
constexpr int TOKEN_SET_RATIO = 16;                // = STRSIM_TOKEN_SET_RATIO
constexpr uint32_t TOKEN_LANE_MAX_BYTES = 64u;     // lane tier: ASCII strings of at most this many bytes ...
constexpr uint32_t TOKEN_LANE_MAX_TOKENS = 16u;    // ... and tokens
constexpr uint32_t TOKEN_WAVE_LDS_TOKENS = 1024u;  // wave tier: descriptors of a row (set form: of both strings) held in LDS
constexpr uint32_t TOKEN_FLAG_ZERO = 1u;           // set form: A or B is empty -> 0.0
constexpr uint32_t TOKEN_FLAG_ONE = 2u;            // set form: A & B is not empty and A - B or B - A is -> 1.0

// What a token call leaves for the host (device block + pinned copy).
struct TokenStatus {
    uint32_t wave_rows[2]; // rows on the work lists of side a / side b (set form: [0] alone)
    uint32_t max_len[2];   // longest row of each column, bytes
    uint32_t begin[2];     // offsets[0] of each column
    uint32_t end[2];       // offsets[rows]
    uint32_t pad[8];
};
static_assert(sizeof(TokenStatus) == 64, "TokenStatus is 64 bytes");

struct TokenSetRec {
    uint32_t sl, la, lb; // scalar values of join(sorted(A & B)), ab, ba
    uint32_t flags;      // TOKEN_FLAG_*
};

// ------------------------------------------------------------------------------------------------
// cores (host and device)
// ------------------------------------------------------------------------------------------------

// Bytes of the whitespace code point that starts at p[i] (i < n), 0 when p[i] does not start one.  Valid UTF-8 is assumed: the lead
// bytes tested (C2, E1, E2, E3) are never continuation bytes, so the answer is 0 in the middle of any character.
STRSIM_HD uint32_t token_space_len(const uint8_t *p, uint32_t i, uint32_t n)
{
    const uint32_t b = p[i];
    if (b < 0x80u) return ((b >= 0x09u && b <= 0x0Du) || (b >= 0x1Cu && b <= 0x20u)) ? 1u : 0u;
    if (b == 0xC2u) return (i + 1u < n && (p[i + 1u] == 0x85u || p[i + 1u] == 0xA0u)) ? 2u : 0u; // U+0085, U+00A0
    if (b < 0xE1u || b > 0xE3u || i + 2u >= n) return 0u;
    const uint32_t c = p[i + 1u], d = p[i + 2u];
    if (b == 0xE1u) return (c == 0x9Au && d == 0x80u) ? 3u : 0u; // U+1680
    if (b == 0xE3u) return (c == 0x80u && d == 0x80u) ? 3u : 0u; // U+3000
    if (c == 0x80u) return ((d >= 0x80u && d <= 0x8Au) || d == 0xA8u || d == 0xA9u || d == 0xAFu) ? 3u : 0u; // U+2000-200A, 2028, 2029, 202F
    return (c == 0x81u && d == 0x9Fu) ? 3u : 0u; // U+205F
}

// Is byte i part of a whitespace code point (its first, second or third byte)?
STRSIM_HD bool token_space_byte(const uint8_t *p, uint32_t i, uint32_t n)
{
    if (token_space_len(p, i, n) != 0u) return true;
    if (p[i] < 0x80u) return false;
    if (i >= 1u && token_space_len(p, i - 1u, n) >= 2u) return true;
    return i >= 2u && token_space_len(p, i - 2u, n) >= 3u;
}

// Does a token start at byte i?  (What a lane of the wave tier asks about its byte.)
STRSIM_HD bool token_is_start(const uint8_t *p, uint32_t i, uint32_t n)
{
    if (token_space_byte(p, i, n)) return false;
    return i == 0u || token_space_byte(p, i - 1u, n);
}

// The end of the token that starts at s: the next whitespace code point, or n.
STRSIM_HD uint32_t token_end(const uint8_t *p, uint32_t s, uint32_t n)
{
    uint32_t e = s;
    while (e < n && token_space_len(p, e, n) == 0u) ++e;
    return e;
}

// scalar values of l bytes of valid UTF-8
STRSIM_HD uint32_t token_chars(const uint8_t *p, uint32_t l)
{
    uint32_t c = 0u;
    for (uint32_t i = 0u; i < l; ++i) c += (p[i] & 0xC0u) != 0x80u;
    return c;
}

// < 0, 0, > 0: bytewise order, a proper prefix first
STRSIM_HD int token_cmp(const uint8_t *x, uint32_t lx, const uint8_t *y, uint32_t ly)
{
    const uint32_t m = lx < ly ? lx : ly;
    for (uint32_t i = 0u; i < m; ++i)
        if (x[i] != y[i]) return x[i] < y[i] ? -1 : 1;
    return lx == ly ? 0 : (lx < ly ? -1 : 1);
}

// A descriptor store D has  void set(uint32_t i, uint32_t start, uint32_t len)  and  void get(uint32_t i, uint32_t &start,
// uint32_t &len) const.  A writer W has  void put(uint32_t pos, uint8_t byte)  and  void copy(uint32_t pos, const uint8_t *src,
// uint32_t len).

struct TokenCountWriter { // the measuring pass: nothing is written
    STRSIM_HD void put(uint32_t, uint8_t) {}
    STRSIM_HD void copy(uint32_t, const uint8_t *, uint32_t) {}
};

struct TokenSerialWriter { // one string per lane, and the host
    uint8_t *out;
    STRSIM_HD void put(uint32_t pos, uint8_t b) { out[pos] = b; }
    STRSIM_HD void copy(uint32_t pos, const uint8_t *src, uint32_t l)
    {
        for (uint32_t k = 0u; k < l; ++k) out[pos + k] = src[k];
    }
};

// The tokens of p[0, n) in order of appearance into d[base ...], at most cap of them; returns how many there are (also beyond cap).
// hi collects the bytes seen (the caller's ASCII test).
template <class D>
STRSIM_HD uint32_t token_split(const uint8_t *p, uint32_t n, D &d, uint32_t base, uint32_t cap, uint32_t &hi)
{
    uint32_t cnt = 0u, i = 0u;
    while (i < n) {
        hi |= p[i];
        const uint32_t w = token_space_len(p, i, n);
        if (w != 0u) { i += w; continue; }
        const uint32_t s = i;
        while (i < n && token_space_len(p, i, n) == 0u) { hi |= p[i]; ++i; }
        if (cnt < cap) d.set(base + cnt, s, i - s);
        ++cnt;
    }
    return cnt;
}

// insertion sort of d[base, base + cnt) (the lane tier: at most TOKEN_LANE_MAX_TOKENS descriptors)
template <class D>
STRSIM_HD void token_isort(const uint8_t *p, D &d, uint32_t base, uint32_t cnt)
{
    for (uint32_t i = 1u; i < cnt; ++i) {
        uint32_t s, l;
        d.get(base + i, s, l);
        uint32_t j = i;
        while (j > 0u) {
            uint32_t s2, l2;
            d.get(base + j - 1u, s2, l2);
            if (token_cmp(p + s2, l2, p + s, l) <= 0) break;
            d.set(base + j, s2, l2);
            --j;
        }
        d.set(base + j, s, l);
    }
}

// One stage of the sorting network over d[base, base + cnt): element i is compared with i ^ (k - 1) in the first stage of a merge
// (j == k / 2) and with i ^ j in the others, and the smaller one always goes to the lower index.  With every comparator pointing
// the same way the padding up to a power of two (+infinity at the top) would never move, so it is not stored: a partner at or
// beyond cnt is skipped.  The comparators of a stage are disjoint; `lane` of `lanes` takes every lanes-th element.
template <class D>
STRSIM_HD void token_net_stage(const uint8_t *p, D &d, uint32_t base, uint32_t cnt, uint32_t k, uint32_t j, uint32_t lane, uint32_t lanes)
{
    for (uint32_t i = lane; i < cnt; i += lanes) {
        const uint32_t l = (j == (k >> 1)) ? (i ^ (k - 1u)) : (i ^ j);
        if (l <= i || l >= cnt) continue;
        uint32_t s1, l1, s2, l2;
        d.get(base + i, s1, l1);
        d.get(base + l, s2, l2);
        if (token_cmp(p + s1, l1, p + s2, l2) > 0) {
            d.set(base + i, s2, l2);
            d.set(base + l, s1, l1);
        }
    }
}

// The whole network; sync() separates the stages (a barrier on the device, nothing on the host with lanes == 1).
template <class D, class Sync>
STRSIM_HD void token_net_sort(const uint8_t *p, D &d, uint32_t base, uint32_t cnt, uint32_t lane, uint32_t lanes, Sync sync)
{
    for (uint32_t k = 2u; (k >> 1) < cnt; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            token_net_stage(p, d, base, cnt, k, j, lane, lanes);
            sync();
        }
}

// join of d[base, base + cnt) through w; returns the bytes
template <class D, class W>
STRSIM_HD uint32_t token_join(const uint8_t *p, const D &d, uint32_t base, uint32_t cnt, W &w)
{
    uint32_t pos = 0u;
    for (uint32_t t = 0u; t < cnt; ++t) {
        uint32_t s, l;
        d.get(base + t, s, l);
        if (t != 0u) { w.put(pos, 0x20u); ++pos; }
        w.copy(pos, p + s, l);
        pos += l;
    }
    return pos;
}

// index of the next token of the sorted list d[base, base + cnt) that differs from token i (duplicates are skipped: sets)
template <class D>
STRSIM_HD uint32_t token_next_distinct(const uint8_t *p, const D &d, uint32_t base, uint32_t cnt, uint32_t i)
{
    uint32_t s, l;
    d.get(base + i, s, l);
    uint32_t j = i + 1u;
    while (j < cnt) {
        uint32_t s2, l2;
        d.get(base + j, s2, l2);
        if (token_cmp(p + s, l, p + s2, l2) != 0) break;
        ++j;
    }
    return j;
}

// The set form of one pair: the sorted lists of a (d[base_a ...], na tokens) and b are merged; A - B is joined through wa, B - A
// through wb; bytes_ab / bytes_ba are what was (or would be) written.
template <class D, class WA, class WB>
STRSIM_HD TokenSetRec token_set_merge(const uint8_t *pa, const uint8_t *pb, const D &d, uint32_t base_a, uint32_t na, uint32_t base_b,
                                      uint32_t nb, WA &wa, WB &wb, uint32_t &bytes_ab, uint32_t &bytes_ba)
{
    uint32_t i = 0u, j = 0u, n_sect = 0u, n_ab = 0u, n_ba = 0u, c_sect = 0u, c_ab = 0u, c_ba = 0u, pos_a = 0u, pos_b = 0u;
    while (i < na || j < nb) {
        uint32_t sa = 0u, la = 0u, sb = 0u, lb = 0u;
        if (i < na) d.get(base_a + i, sa, la);
        if (j < nb) d.get(base_b + j, sb, lb);
        const int c = i >= na ? 1 : (j >= nb ? -1 : token_cmp(pa + sa, la, pb + sb, lb));
        if (c < 0) {
            if (n_ab != 0u) { wa.put(pos_a, 0x20u); ++pos_a; }
            wa.copy(pos_a, pa + sa, la);
            pos_a += la;
            c_ab += token_chars(pa + sa, la);
            ++n_ab;
        } else if (c > 0) {
            if (n_ba != 0u) { wb.put(pos_b, 0x20u); ++pos_b; }
            wb.copy(pos_b, pb + sb, lb);
            pos_b += lb;
            c_ba += token_chars(pb + sb, lb);
            ++n_ba;
        } else {
            c_sect += token_chars(pa + sa, la);
            ++n_sect;
        }
        if (c <= 0) i = token_next_distinct(pa, d, base_a, na, i);
        if (c >= 0) j = token_next_distinct(pb, d, base_b, nb, j);
    }
    bytes_ab = pos_a;
    bytes_ba = pos_b;
    TokenSetRec r;
    r.sl = n_sect ? c_sect + n_sect - 1u : 0u;
    r.la = n_ab ? c_ab + n_ab - 1u : 0u;
    r.lb = n_ba ? c_ba + n_ba - 1u : 0u;
    r.flags = (na == 0u || nb == 0u) ? TOKEN_FLAG_ZERO : ((n_sect != 0u && (n_ab == 0u || n_ba == 0u)) ? TOKEN_FLAG_ONE : 0u);
    return r;
}

// The rule of token_set_ratio; d = indel_distance(ab, ba).  E(d, s) is epilogue_indel: 1.0 when s == 0, else 1.0 - d / s.
STRSIM_HD double token_set_score(const TokenSetRec &r, uint32_t d)
{
    if (r.flags & TOKEN_FLAG_ZERO) return 0.0;
    if (r.flags & TOKEN_FLAG_ONE) return 1.0;
    const uint64_t sep = r.sl != 0u ? 1u : 0u;
    const uint64_t sab = (uint64_t)r.sl + sep + r.la, sba = (uint64_t)r.sl + sep + r.lb;
    const double r0 = epilogue_indel(d, sab, sba);
    if (r.sl == 0u) return r0;
    const double r1 = epilogue_indel(sep + r.la, r.sl, sab), r2 = epilogue_indel(sep + r.lb, r.sl, sba);
    const double m = r1 > r2 ? r1 : r2;
    return r0 > m ? r0 : m;
}

// descriptors of the wave tier and of the host: (start, length) pairs
struct TokenPairStore {
    uint32_t *d; // 2 words per descriptor
    STRSIM_HD void set(uint32_t i, uint32_t s, uint32_t l) { d[2u * i] = s; d[2u * i + 1u] = l; }
    STRSIM_HD void get(uint32_t i, uint32_t &s, uint32_t &l) const { s = d[2u * i]; l = d[2u * i + 1u]; }
};

// descriptor words a wave needs for a row of n bytes: a token and the whitespace behind it take two bytes at least
STRSIM_HD uint64_t token_max_tokens(uint64_t n) { return (n + 1u) / 2u; }

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

constexpr int TOKEN_THREADS = 256;

// descriptors of the lane tier: start and length in a byte each (both <= 64), LDS as [slot][thread]
struct TokenLaneStore {
    uint16_t *s; // + threadIdx.x
    STRSIM_HD void set(uint32_t i, uint32_t st, uint32_t l) { s[i * TOKEN_THREADS] = (uint16_t)(st | (l << 8)); }
    STRSIM_HD void get(uint32_t i, uint32_t &st, uint32_t &l) const
    {
        const uint32_t v = s[i * TOKEN_THREADS];
        st = v & 0xFFu;
        l = v >> 8;
    }
};

struct TokenWaveWriter { // every lane of the wave is at the same token: the bytes go 64 at a time
    uint8_t *out;
    uint32_t lane;
    STRSIM_HD void put(uint32_t pos, uint8_t b) { if (lane == 0u) out[pos] = b; }
    STRSIM_HD void copy(uint32_t pos, const uint8_t *src, uint32_t l)
    {
        for (uint32_t k = lane; k < l; k += 64u) out[pos + k] = src[k];
    }
};

// The longest row of a column and its first and last offset (side 0 or 1 of st; max_len zeroed before the launch).
__global__ __launch_bounds__(TOKEN_THREADS) void k_token_bounds(const uint32_t *__restrict__ off, uint64_t rows, TokenStatus *st, int side)
{
    uint32_t m = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = off[i + 1] - off[i];
        m = l > m ? l : m;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, d, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63u) == 0u && m != 0u) atomicMax(&st->max_len[side], m);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->begin[side] = off[0];
        st->end[side] = off[rows];
    }
}

// ---- sort form ----

// One string per lane.  WRITE = false: out_off[row + 1] = the bytes of the row's normalised string (out_off[0] = 0), rows this
// tier cannot take go to `list` (counted in *count).  WRITE = true: out_off holds the offsets, the strings go to out_val.
template <bool WRITE>
__global__ __launch_bounds__(TOKEN_THREADS) void k_token_sort_lane(const uint32_t *__restrict__ off, const uint8_t *__restrict__ val, uint64_t rows,
                                                                   uint32_t *__restrict__ out_off, uint8_t *__restrict__ out_val,
                                                                   uint32_t *__restrict__ list, uint32_t *count)
{
    __shared__ uint16_t s_desc[TOKEN_LANE_MAX_TOKENS * TOKEN_THREADS];
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = row < rows;
    const uint32_t o0 = live ? off[row] : 0u, len = live ? off[row + 1] - o0 : 0u;
    const bool fits = live && len <= TOKEN_LANE_MAX_BYTES;
    const uint8_t *p = val + o0;
    TokenLaneStore d{s_desc + threadIdx.x};
    uint32_t hi = 0u;
    const uint32_t cnt = token_split(p, fits ? len : 0u, d, 0u, TOKEN_LANE_MAX_TOKENS, hi);
    const bool ok = fits && (hi & 0x80u) == 0u && cnt <= TOKEN_LANE_MAX_TOKENS;
    if constexpr (!WRITE) {
        if (row == 0) out_off[0] = 0u;
        if (ok) {
            TokenCountWriter w;
            out_off[row + 1] = token_join(p, d, 0u, cnt, w);
        }
        wave_append(live && !ok, (uint32_t)row, list, count);
    } else if (ok) {
        token_isort(p, d, 0u, cnt);
        TokenSerialWriter w{out_val + out_off[row]};
        token_join(p, d, 0u, cnt, w);
    }
}

// the tokens of p[0, n) into d[base ...] by the whole wave; returns their count (wave-uniform)
__device__ __forceinline__ uint32_t token_split_wave(const uint8_t *p, uint32_t n, TokenPairStore &d, uint32_t base, uint32_t lane)
{
    uint32_t cnt = 0u;
    for (uint32_t b0 = 0u; b0 < n; b0 += 64u) {
        const uint32_t i = b0 + lane;
        const bool st = i < n && token_is_start(p, i, n);
        const uint64_t m = __ballot(st);
        if (st) d.set(base + cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), i, token_end(p, i, n) - i);
        cnt += (uint32_t)__popcll(m);
    }
    return cnt;
}

// One string per wave (blockDim.x = 64) for the rows of `list` (*count of them).  scratch: gridDim.x slots of slot_words words for
// rows that can hold more than TOKEN_WAVE_LDS_TOKENS tokens (nullptr when the column has none).
template <bool WRITE>
__global__ __launch_bounds__(64) void k_token_sort_wave(const uint32_t *__restrict__ off, const uint8_t *__restrict__ val,
                                                        uint32_t *__restrict__ out_off, uint8_t *__restrict__ out_val,
                                                        const uint32_t *__restrict__ list, const uint32_t *count, uint32_t *scratch,
                                                        uint64_t slot_words)
{
    __shared__ uint32_t s_desc[2u * TOKEN_WAVE_LDS_TOKENS];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t rows = *count;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const uint32_t row = list[r];
        const uint32_t o0 = off[row], n = off[row + 1] - o0;
        const uint8_t *p = val + o0;
        TokenPairStore d{token_max_tokens(n) <= TOKEN_WAVE_LDS_TOKENS ? s_desc : scratch + (uint64_t)blockIdx.x * slot_words};
        const uint32_t cnt = token_split_wave(p, n, d, 0u, lane);
        __syncthreads();
        if constexpr (!WRITE) {
            TokenCountWriter w;
            const uint32_t bytes = token_join(p, d, 0u, cnt, w);
            if (lane == 0u) out_off[row + 1] = bytes;
        } else {
            token_net_sort(p, d, 0u, cnt, lane, 64u, [] { __syncthreads(); });
            TokenWaveWriter w{out_val + out_off[row], lane};
            token_join(p, d, 0u, cnt, w);
        }
        __syncthreads(); // (the next row overwrites the descriptors)
    }
}

// ---- set form ----

// One pair per lane; rows_a / rows_b == 1: that side is a literal.  WRITE = false: off_ab[row + 1] / off_ba[row + 1] = the bytes of
// ab / ba, rec[row] the record, other rows to `list`.  WRITE = true: the strings go to val_ab / val_ba.
template <bool WRITE>
__global__ __launch_bounds__(TOKEN_THREADS) void k_token_set_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rows_a,
                                                                  const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rows_b,
                                                                  uint64_t n, uint32_t *__restrict__ off_ab, uint8_t *__restrict__ val_ab,
                                                                  uint32_t *__restrict__ off_ba, uint8_t *__restrict__ val_ba,
                                                                  TokenSetRec *__restrict__ rec, uint32_t *__restrict__ list, uint32_t *count)
{
    __shared__ uint16_t s_desc[2u * TOKEN_LANE_MAX_TOKENS * TOKEN_THREADS];
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = row < n;
    const uint64_t ia = (rows_a == 1 || !live) ? 0 : row, ib = (rows_b == 1 || !live) ? 0 : row;
    const uint32_t a0 = offA[ia], la = offA[ia + 1] - a0;
    const uint32_t b0 = offB[ib], lb = offB[ib + 1] - b0;
    const bool fits = live && la <= TOKEN_LANE_MAX_BYTES && lb <= TOKEN_LANE_MAX_BYTES;
    const uint8_t *pa = valA + a0, *pb = valB + b0;
    TokenLaneStore d{s_desc + threadIdx.x};
    uint32_t hi = 0u;
    const uint32_t na = token_split(pa, fits ? la : 0u, d, 0u, TOKEN_LANE_MAX_TOKENS, hi);
    const uint32_t nb = token_split(pb, fits ? lb : 0u, d, TOKEN_LANE_MAX_TOKENS, TOKEN_LANE_MAX_TOKENS, hi);
    const bool ok = fits && (hi & 0x80u) == 0u && na <= TOKEN_LANE_MAX_TOKENS && nb <= TOKEN_LANE_MAX_TOKENS;
    if constexpr (!WRITE) {
        if (row == 0) { off_ab[0] = 0u; off_ba[0] = 0u; }
        wave_append(live && !ok, (uint32_t)row, list, count);
    }
    if (!ok) return;
    token_isort(pa, d, 0u, na);
    token_isort(pb, d, TOKEN_LANE_MAX_TOKENS, nb);
    uint32_t bytes_ab, bytes_ba;
    if constexpr (!WRITE) {
        TokenCountWriter wa, wb;
        rec[row] = token_set_merge(pa, pb, d, 0u, na, TOKEN_LANE_MAX_TOKENS, nb, wa, wb, bytes_ab, bytes_ba);
        off_ab[row + 1] = bytes_ab;
        off_ba[row + 1] = bytes_ba;
    } else {
        TokenSerialWriter wa{val_ab + off_ab[row]}, wb{val_ba + off_ba[row]};
        token_set_merge(pa, pb, d, 0u, na, TOKEN_LANE_MAX_TOKENS, nb, wa, wb, bytes_ab, bytes_ba);
    }
}

// One pair per wave for the rows of `list`; scratch as k_token_sort_wave (a slot holds the descriptors of both strings).
template <bool WRITE>
__global__ __launch_bounds__(64) void k_token_set_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rows_a,
                                                       const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rows_b,
                                                       uint32_t *__restrict__ off_ab, uint8_t *__restrict__ val_ab,
                                                       uint32_t *__restrict__ off_ba, uint8_t *__restrict__ val_ba,
                                                       TokenSetRec *__restrict__ rec, const uint32_t *__restrict__ list, const uint32_t *count,
                                                       uint32_t *scratch, uint64_t slot_words)
{
    __shared__ uint32_t s_desc[2u * TOKEN_WAVE_LDS_TOKENS];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t rows = *count;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const uint32_t row = list[r];
        const uint64_t ia = rows_a == 1 ? 0 : row, ib = rows_b == 1 ? 0 : row;
        const uint32_t a0 = offA[ia], la = offA[ia + 1] - a0;
        const uint32_t b0 = offB[ib], lb = offB[ib + 1] - b0;
        const uint8_t *pa = valA + a0, *pb = valB + b0;
        const bool lds = token_max_tokens(la) + token_max_tokens(lb) <= TOKEN_WAVE_LDS_TOKENS;
        TokenPairStore d{lds ? s_desc : scratch + (uint64_t)blockIdx.x * slot_words};
        const uint32_t na = token_split_wave(pa, la, d, 0u, lane);
        const uint32_t nb = token_split_wave(pb, lb, d, na, lane);
        __syncthreads();
        token_net_sort(pa, d, 0u, na, lane, 64u, [] { __syncthreads(); });
        token_net_sort(pb, d, na, nb, lane, 64u, [] { __syncthreads(); });
        uint32_t bytes_ab, bytes_ba;
        if constexpr (!WRITE) {
            TokenCountWriter wa, wb;
            const TokenSetRec rr = token_set_merge(pa, pb, d, 0u, na, na, nb, wa, wb, bytes_ab, bytes_ba);
            if (lane == 0u) {
                rec[row] = rr;
                off_ab[row + 1] = bytes_ab;
                off_ba[row + 1] = bytes_ba;
            }
        } else {
            TokenWaveWriter wa{val_ab + off_ab[row], lane}, wb{val_ba + off_ba[row], lane};
            token_set_merge(pa, pb, d, 0u, na, na, nb, wa, wb, bytes_ab, bytes_ba);
        }
        __syncthreads();
    }
}

// out[row] = the rule of token_set_ratio over the record and d32[row] = indel_distance(ab, ba)
__global__ __launch_bounds__(TOKEN_THREADS) void k_token_set_epilogue(const TokenSetRec *__restrict__ rec, const uint32_t *__restrict__ d32,
                                                                      double *__restrict__ out, uint64_t n)
{
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row < n) out[row] = token_set_score(rec[row], d32[row]);
}

// ---- offsets from lengths: an inclusive scan of x[0, n) in place, three launches ----
// (x = out_off + 1: out_off[i + 1] holds the bytes of row i and becomes the end of row i)
constexpr int TOKEN_SCAN_PER_THREAD = 16, TOKEN_SCAN_BLOCK = TOKEN_THREADS * TOKEN_SCAN_PER_THREAD;

// the exclusive prefix of v over the workgroup; *total = the workgroup's sum
__device__ __forceinline__ uint32_t token_block_exclusive(uint32_t v, uint32_t *s_wave, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= (uint32_t)d) inc += up;
    }
    if (lane == 63u) s_wave[wv] = inc;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
    for (uint32_t w = 0u; w < (uint32_t)TOKEN_THREADS / 64u; ++w) {
        if (w < wv) before += s_wave[w];
        all += s_wave[w];
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(TOKEN_THREADS) void k_token_scan_sums(const uint32_t *__restrict__ x, uint64_t n, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t s_wave[TOKEN_THREADS / 64];
    const uint64_t at = (uint64_t)blockIdx.x * TOKEN_SCAN_BLOCK + (uint64_t)threadIdx.x * TOKEN_SCAN_PER_THREAD;
    uint32_t v = 0u;
    for (int k = 0; k < TOKEN_SCAN_PER_THREAD; ++k)
        if (at + k < n) v += x[at + k];
    uint32_t total;
    token_block_exclusive(v, s_wave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0, nb) -> their exclusive prefixes, by one workgroup (every thread a contiguous part)
__global__ __launch_bounds__(TOKEN_THREADS) void k_token_scan_top(uint32_t *__restrict__ sums, uint32_t nb)
{
    __shared__ uint32_t s_wave[TOKEN_THREADS / 64];
    const uint32_t per = (nb + TOKEN_THREADS - 1u) / TOKEN_THREADS;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    uint32_t v = 0u;
    for (uint32_t i = lo; i < hi; ++i) v += sums[i];
    uint32_t total;
    uint32_t run = token_block_exclusive(v, s_wave, &total);
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t s = sums[i];
        sums[i] = run;
        run += s;
    }
}

__global__ __launch_bounds__(TOKEN_THREADS) void k_token_scan_apply(uint32_t *__restrict__ x, uint64_t n, const uint32_t *__restrict__ sums)
{
    __shared__ uint32_t s_wave[TOKEN_THREADS / 64];
    const uint64_t at = (uint64_t)blockIdx.x * TOKEN_SCAN_BLOCK + (uint64_t)threadIdx.x * TOKEN_SCAN_PER_THREAD;
    uint32_t v[TOKEN_SCAN_PER_THREAD], tot = 0u;
#pragma unroll
    for (int k = 0; k < TOKEN_SCAN_PER_THREAD; ++k) {
        v[k] = at + k < n ? x[at + k] : 0u;
        tot += v[k];
    }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + token_block_exclusive(tot, s_wave, &total);
#pragma unroll
    for (int k = 0; k < TOKEN_SCAN_PER_THREAD; ++k) {
        run += v[k];
        if (at + k < n) x[at + k] = run;
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
