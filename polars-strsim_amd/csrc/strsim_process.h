// strsim_process.h -- default_process: rapidfuzz's utils.default_process made context-free, as a column transform on the device.
//
// Every scalar value c of a row is mapped by m: m(c) = U+0020 when c is neither alphanumeric (str.isalnum) nor "_", else the first
// scalar value of c.lower(); then U+0020 is removed from both ends of the row (inner runs of spaces stay).  Below U+0080 m is
// arithmetic (process_map_ascii), at and above it a two-stage table generated from Python (strsim_process_table.h).  A processed
// row can be longer than its input: U+023A and U+023E map from two bytes of UTF-8 to three, so bytes + bytes / 2 always suffices.
//
// The transform runs twice, like the token transforms it sits beside (strsim_token.h, DESIGN.md sections 16 and 19): a measuring
// pass leaves the output lengths, the offset scan (k_token_scan_*) turns them into offsets, a writing pass fills the values.
//   k_process_lane  one string per lane: ASCII rows of at most PROCESS_LANE_MAX_BYTES bytes.  Measuring finds the first and the
//                   last byte that does not map to a space; writing maps whole dwords (process_map_ascii_word) where the
//                   destination is aligned, bytes at its ends.  Every other row goes to a work list (wave_append).
//   k_process_wave  one string per wave for the work list: any UTF-8, any length.  64 bytes at a time, a lane per byte: a lane on
//                   a start byte decodes, maps and knows its output length; ballots give every lane its position (the output
//                   lengths are 1 .. 4, so four ballots are the prefix sum) and the first and last kept scalar value.  The bytes
//                   of a chunk are put together in LDS and leave in aligned dwords.
// Malformed UTF-8 gives an unspecified string, but no read leaves the row's bytes and no write its output slot or the wave's LDS
// words: process_decode turns a lead byte without its continuation bytes (cut off by the row's end included) into a space, so
// the output of any bytes is bounded as that of valid UTF-8 is, and a scalar value is written only where it fits in whole.
// The row functions below are host/device code: tests/cpu_harness/process_harness.cpp compiles them with g++.
#pragma once
#include <stdint.h>

#include "strsim_token.h"
#include "strsim_process_table.h"

namespace strsim {

constexpr int PROCESS_DEFAULT = 1;                  // = STRSIM_PROCESS_DEFAULT
constexpr uint32_t PROCESS_LANE_MAX_BYTES = 64u;    // lane tier: ASCII rows of at most this many bytes

// the table as the kernels and the host see it (device or host pointers)
struct ProcessTable {
    const uint8_t *block; // PROCESS_BLOCK
    const uint8_t *cls;   // PROCESS_CLASS
    const int32_t *delta; // PROCESS_DELTA
};
constexpr size_t PROCESS_TABLE_CLASS_AT = sizeof(PROCESS_BLOCK);
constexpr size_t PROCESS_TABLE_DELTA_AT = PROCESS_TABLE_CLASS_AT + sizeof(PROCESS_CLASS);
constexpr size_t PROCESS_TABLE_BYTES = PROCESS_TABLE_DELTA_AT + sizeof(PROCESS_DELTA);
static_assert(PROCESS_TABLE_DELTA_AT % 4u == 0u, "the deltas are read as words");

// ------------------------------------------------------------------------------------------------
// row functions (host and device)
// ------------------------------------------------------------------------------------------------

// m below U+0080: A-Z + 32, a-z 0-9 _ kept, everything else (NUL included) a space.  (A byte at or above 0x80 gives a space.)
STRSIM_HD uint32_t process_map_ascii(uint32_t b)
{
    if (b - 0x41u < 26u) return b + 32u;
    return (b - 0x61u < 26u || b - 0x30u < 10u || b == 0x5Fu) ? b : 0x20u;
}

// the same for four ASCII bytes in a word: b + k sets a byte's top bit exactly when b >= 0x80 - k, and nothing carries between
// bytes below 0x80
STRSIM_HD uint32_t process_map_ascii_word(uint32_t w)
{
    const uint32_t top = 0x80808080u;
    const uint32_t upper = (w + 0x3F3F3F3Fu) & ~(w + 0x25252525u) & top; // 0x41 .. 0x5A
    const uint32_t lower = (w + 0x1F1F1F1Fu) & ~(w + 0x05050505u) & top; // 0x61 .. 0x7A
    const uint32_t digit = (w + 0x50505050u) & ~(w + 0x46464646u) & top; // 0x30 .. 0x39
    const uint32_t under = (w + 0x21212121u) & ~(w + 0x20202020u) & top; // 0x5F
    const uint32_t keep = ((upper | lower | digit | under) >> 7) * 0xFFu;
    return ((w | (upper >> 2)) & keep) | (0x20202020u & ~keep);
}

// m of any value: surrogates (by the table) and values above U+10FFFF map to U+0020
STRSIM_HD uint32_t process_map(uint32_t cp, const ProcessTable &t)
{
    if (cp < 0x80u) return process_map_ascii(cp);
    if (cp > 0x10FFFFu) return 0x20u;
    const uint32_t c = t.cls[(uint32_t)t.block[cp >> 8] * 256u + (cp & 0xFFu)];
    if (c == 0u) return cp;
    return c == 1u ? 0x20u : (uint32_t)((int32_t)cp + t.delta[c - 2u]);
}

// The scalar value of the sequence that starts at p[i] (i < n; p[i] is not a continuation byte).  The lead byte gives the length;
// when one of the continuation bytes it calls for is missing -- the row ends first, or the byte there is not 10xxxxxx -- or the
// lead byte is none (0xF8 and above), the byte counts as U+0020 on its own.  Bytes at or beyond n are not read.  So a scalar value
// of more than one output byte always owns as many input bytes as its lead byte says: any bytes at all process to at most
// bytes + bytes / 2, and the start bytes of 64 consecutive bytes to at most 98 (31 two-byte values that grow to three, one byte,
// and a four-byte lead in the last place).
STRSIM_HD uint32_t process_decode(const uint8_t *p, uint32_t i, uint32_t n)
{
    const uint32_t b0 = p[i];
    if (b0 < 0x80u) return b0;
    const uint32_t len = b0 < 0xE0u ? 2u : (b0 < 0xF0u ? 3u : 4u);
    if (b0 >= 0xF8u || i + len > n) return 0x20u;
    uint32_t cp = b0 & (0x7Fu >> len);
    for (uint32_t k = 1u; k < len; ++k) {
        const uint32_t c = p[i + k];
        if ((c & 0xC0u) != 0x80u) return 0x20u;
        cp = (cp << 6) | (c & 0x3Fu);
    }
    return cp;
}

STRSIM_HD uint32_t process_utf8_len(uint32_t cp) { return cp < 0x80u ? 1u : (cp < 0x800u ? 2u : (cp < 0x10000u ? 3u : 4u)); }

// the UTF-8 of cp (l = process_utf8_len(cp) bytes), first byte lowest
STRSIM_HD uint32_t process_utf8_pack(uint32_t cp, uint32_t l)
{
    if (l == 1u) return cp;
    if (l == 2u) return (0xC0u | (cp >> 6)) | ((0x80u | (cp & 0x3Fu)) << 8);
    if (l == 3u) return (0xE0u | (cp >> 12)) | ((0x80u | ((cp >> 6) & 0x3Fu)) << 8) | ((0x80u | (cp & 0x3Fu)) << 16);
    return (0xF0u | (cp >> 18)) | ((0x80u | ((cp >> 12) & 0x3Fu)) << 8) | ((0x80u | ((cp >> 6) & 0x3Fu)) << 16) | ((0x80u | (cp & 0x3Fu)) << 24);
}

// Lane tier, measuring: the processed length of the ASCII row p[0, n); first = where its first kept byte is, hi = every byte
// ORed together (the caller's ASCII test: with a byte at or above 0x80 the result means nothing).  Whole aligned dwords inside
// the row, bytes at its ends.
STRSIM_HD uint32_t process_ascii_measure(const uint8_t *p, uint32_t n, uint32_t &first, uint32_t &hi)
{
    uint32_t f = n, l = 0u, i = 0u, h = 0u;
    auto one = [&](uint32_t b, uint32_t at) {
        h |= b;
        if (process_map_ascii(b) != 0x20u) {
            if (f == n) f = at;
            l = at + 1u;
        }
    };
    for (; i < n && ((uintptr_t)(p + i) & 3u) != 0u; ++i) one(p[i], i);
    for (; i + 4u <= n; i += 4u) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(p + i);
        h |= w & 0x80808080u;
        if (process_map_ascii_word(w & 0x7F7F7F7Fu) == 0x20202020u) continue; // (four spaces: nothing to note)
        for (uint32_t k = 0u; k < 4u; ++k) one((w >> (8u * k)) & 0xFFu, i + k);
    }
    for (; i < n; ++i) one(p[i], i);
    hi = h;
    first = f;
    return f == n ? 0u : l - f;
}

// Lane tier, writing: dst[0, len) = m of the ASCII bytes src[0, len).  The destination is written in aligned dwords (bytes up to
// the first and behind the last one); a source dword is loaded whole when it is aligned too.
STRSIM_HD void process_ascii_write(const uint8_t *src, uint8_t *dst, uint32_t len)
{
    uint32_t i = 0u;
    for (; i < len && ((uintptr_t)(dst + i) & 3u) != 0u; ++i) dst[i] = (uint8_t)process_map_ascii(src[i]);
    const bool whole = ((uintptr_t)(src + i) & 3u) == 0u;
    for (; i + 4u <= len; i += 4u) {
        const uint32_t w = whole ? *reinterpret_cast<const uint32_t *>(src + i)
                                 : ((uint32_t)src[i] | ((uint32_t)src[i + 1u] << 8) | ((uint32_t)src[i + 2u] << 16) | ((uint32_t)src[i + 3u] << 24));
        *reinterpret_cast<uint32_t *>(dst + i) = process_map_ascii_word(w);
    }
    for (; i < len; ++i) dst[i] = (uint8_t)process_map_ascii(src[i]);
}

// Wave tier, writing.  A row's destination is seen from the aligned address at or below it: base = dst - a with a = dst & 3, and
// the row's bytes are the positions [a, end) behind base.  Word k of that view goes out as a dword when all four of its bytes are
// the row's, byte by byte otherwise (the first and the last word of a row).
STRSIM_HD void process_put_word(uint8_t *base, uint32_t k, uint32_t w, uint32_t a, uint32_t end)
{
    const uint32_t lo = 4u * k;
    if (lo >= a && lo + 4u <= end) {
        *reinterpret_cast<uint32_t *>(base + lo) = w;
        return;
    }
    for (uint32_t b = 0u; b < 4u; ++b)
        if (lo + b >= a && lo + b < end) base[lo + b] = (uint8_t)(w >> (8u * b));
}

// What the wave knows of a row while it walks it, 64 bytes at a time (wave-uniform).
struct ProcessWalk {
    uint32_t cum;   // output bytes of the scalar values before this chunk, spaces at the front included
    uint32_t lead;  // scalar values in front of the first kept one (all of them spaces: a byte each)
    uint32_t trail; // ... and behind the last kept one so far
    bool seen;      // a kept scalar value has been met
};

// The chunk's part of the walk.  sm: the lanes on a start byte; km: those whose scalar value is kept (does not map to a space);
// tot: the output bytes of the chunk's scalar values.
STRSIM_HD void process_walk_chunk(ProcessWalk &w, uint64_t sm, uint64_t km, uint32_t tot)
{
    auto pop = [](uint64_t v) { return (uint32_t)__builtin_popcountll((unsigned long long)v); };
    if (km != 0ull) {
        if (!w.seen) {
            w.lead = w.cum + pop(sm & ((km & (0ull - km)) - 1ull));
            w.seen = true;
        }
        uint64_t upto = km; // every bit up to the chunk's last kept scalar value
        upto |= upto >> 1; upto |= upto >> 2; upto |= upto >> 4; upto |= upto >> 8; upto |= upto >> 16; upto |= upto >> 32;
        w.trail = pop(sm & ~upto);
    } else if (w.seen) {
        w.trail += pop(sm);
    }
    w.cum += tot;
}

STRSIM_HD uint32_t process_walk_bytes(const ProcessWalk &w) { return w.seen ? w.cum - w.lead - w.trail : 0u; }

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

// One string per lane.  WRITE = false: out_off[row + 1] = the bytes of the processed row (out_off[0] = 0), rows this tier cannot
// take go to `list` (counted in *count).  WRITE = true: out_off holds the offsets, the strings go to out_val.
template <bool WRITE>
__global__ __launch_bounds__(TOKEN_THREADS) void k_process_lane(const uint32_t *__restrict__ off, const uint8_t *__restrict__ val, uint64_t rows,
                                                                uint32_t *__restrict__ out_off, uint8_t *__restrict__ out_val,
                                                                uint32_t *__restrict__ list, uint32_t *count)
{
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = row < rows;
    const uint32_t o0 = live ? off[row] : 0u, len = live ? off[row + 1] - o0 : 0u;
    const bool fits = live && len <= PROCESS_LANE_MAX_BYTES;
    const uint8_t *p = val + o0;
    uint32_t first = 0u, hi = 0u;
    const uint32_t bytes = process_ascii_measure(p, fits ? len : 0u, first, hi);
    const bool ok = fits && (hi & 0x80808080u) == 0u;
    if constexpr (!WRITE) {
        if (row == 0) out_off[0] = 0u;
        if (ok) out_off[row + 1] = bytes;
        wave_append(live && !ok, (uint32_t)row, list, count);
    } else if (ok) {
        process_ascii_write(p + first, out_val + out_off[row], bytes);
    }
}

// One string per wave (blockDim.x = 64) for the rows of `list` (*count of them).
template <bool WRITE>
__global__ __launch_bounds__(64) void k_process_wave(const uint32_t *__restrict__ off, const uint8_t *__restrict__ val,
                                                     uint32_t *__restrict__ out_off, uint8_t *__restrict__ out_val,
                                                     const uint32_t *__restrict__ list, const uint32_t *count, ProcessTable t)
{
    // the output bytes of a chunk behind the bytes of an unfinished dword: at most 3 + 98 for any bytes at all (process_decode)
    __shared__ uint32_t s_w[32];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t rows = *count;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const uint32_t row = list[r];
        const uint32_t o0 = off[row], n = off[row + 1] - o0;
        const uint8_t *p = val + o0;
        uint32_t out_len = 0u, a = 0u;
        uint8_t *base = nullptr;
        if constexpr (WRITE) {
            const uint32_t d0 = out_off[row];
            out_len = out_off[row + 1] - d0;
            a = (uint32_t)((uintptr_t)(out_val + d0) & 3u);
            base = out_val + d0 - a;
        }
        const uint32_t end = a + out_len;
        uint32_t v0 = a; // WRITE: the position behind base up to which the row's bytes are in s_w or out
        ProcessWalk w{0u, 0u, 0u, false};
        for (uint32_t b0 = 0u; b0 < n; b0 += 64u) {
            const uint32_t i = b0 + lane;
            const bool st = i < n && (p[i] & 0xC0u) != 0x80u;
            uint32_t m = 0x20u, ol = 0u;
            if (st) {
                m = process_map(process_decode(p, i, n), t);
                ol = process_utf8_len(m);
            }
            const uint64_t sm = __ballot(st), km = __ballot(st && m != 0x20u);
            const uint64_t m2 = __ballot(ol >= 2u), m3 = __ballot(ol >= 3u), m4 = __ballot(ol >= 4u);
            const uint32_t at = w.cum + (uint32_t)(__popcll(sm & below) + __popcll(m2 & below) + __popcll(m3 & below) + __popcll(m4 & below));
            process_walk_chunk(w, sm, km, (uint32_t)(__popcll(sm) + __popcll(m2) + __popcll(m3) + __popcll(m4)));
            if constexpr (WRITE) {
                if (!w.seen) continue; // (wave-uniform: nothing but spaces so far)
                // a scalar value goes out when it starts at or behind the first kept one and ends inside the row's output
                if (st && at >= w.lead && at - w.lead + ol <= out_len) {
                    uint8_t *sb = reinterpret_cast<uint8_t *>(s_w) + (a + at - w.lead - (v0 & ~3u));
                    const uint32_t pk = process_utf8_pack(m, ol);
                    for (uint32_t k = 0u; k < ol; ++k) sb[k] = (uint8_t)(pk >> (8u * k));
                }
                __syncthreads();
                uint32_t e = w.cum - w.lead; // (w.cum: this chunk included)
                e = e < out_len ? e : out_len;
                const uint32_t v1 = a + e, w0 = v0 >> 2, nw = (v1 >> 2) - w0;
                if (lane < nw) process_put_word(base, w0 + lane, s_w[lane], a, end);
                __syncthreads();
                if (lane == 0u && nw != 0u) s_w[0] = s_w[nw]; // the bytes of the dword that is not full yet
                __syncthreads();
                v0 = v1;
            }
        }
        if constexpr (!WRITE) {
            if (lane == 0u) out_off[row + 1] = process_walk_bytes(w);
        } else {
            if (lane == 0u && (v0 & 3u) != 0u) process_put_word(base, v0 >> 2, s_w[0], a, end);
            __syncthreads(); // (the next row overwrites s_w)
        }
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
