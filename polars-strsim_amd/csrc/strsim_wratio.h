// strsim_wratio.h -- token_ratio, partial_token_sort_ratio, partial_token_set_ratio, partial_token_ratio and WRatio (measure ids 18,
// 20, 22, 24 and 26): compositions of the Indel, partial-ratio and token flows (strsim_indel.h, strsim_partial.h, strsim_token.h).
//
// What this header adds is what the compositions need beside those flows:
//   k_wratio_classify  a row's class from the lengths of its RAW strings in scalar values -- empty, near (2 hi < 3 lo), far with
//                      hi <= 8 lo, far beyond -- and the row's index appended to the near or the far list (one atomic a wave).
//   k_take_measure /   the rows of a list as a column of their own (offsets + values) in context scratch: lengths, the offset scan
//   k_take_write       of strsim_token.h, then the copy, eight lanes a row, in aligned dwords of the destination.
//   k_wratio_combine   the rule of WRatio per original row from its class and the scores at its list position.
//   k_max_f64, k_partial_token_set_epilogue   the epilogues of ids 18 / 24 and 22.
// The class predicate and the rules are host/device code: tests/cpu_harness/wratio_harness.cpp compiles them with g++.
#pragma once
#include <stdint.h>

#include "strsim_token.h"

namespace strsim {

constexpr int TOKEN_RATIO = 18;              // = STRSIM_TOKEN_RATIO
constexpr int PARTIAL_TOKEN_SORT_RATIO = 20; // = STRSIM_PARTIAL_TOKEN_SORT_RATIO
constexpr int PARTIAL_TOKEN_SET_RATIO = 22;  // = STRSIM_PARTIAL_TOKEN_SET_RATIO
constexpr int PARTIAL_TOKEN_RATIO = 24;      // = STRSIM_PARTIAL_TOKEN_RATIO
constexpr int WRATIO = 26;                   // = STRSIM_WRATIO

constexpr uint32_t WRATIO_EMPTY = 0u; // lo == 0 -> 0.0
constexpr uint32_t WRATIO_NEAR = 1u;  // 2 hi < 3 lo: the token family
constexpr uint32_t WRATIO_FAR8 = 2u;  // hi <= 8 lo: the partial family scaled by 0.9
constexpr uint32_t WRATIO_FAR = 3u;   // the partial family scaled by 0.6

// What a wratio call leaves for the host (device block + pinned copy).
struct WratioStatus {
    uint32_t rows[2]; // rows on the near / the far list
    uint32_t pad[2];
};

// ------------------------------------------------------------------------------------------------
// cores (host and device)
// ------------------------------------------------------------------------------------------------

// the class of a pair from the lengths of its raw strings in scalar values (integer comparisons only)
STRSIM_HD uint32_t wratio_class(uint32_t la, uint32_t lb)
{
    const uint64_t lo = la < lb ? la : lb, hi = la < lb ? lb : la;
    if (lo == 0u) return WRATIO_EMPTY;
    if (2u * hi < 3u * lo) return WRATIO_NEAR;
    return hi <= 8u * lo ? WRATIO_FAR8 : WRATIO_FAR;
}

STRSIM_HD double wratio_max(double x, double y) { return y > x ? y : x; }

// The rule of WRatio.  r = indel(a, b); near: s0 = token_ratio; far: s0 = partial_ratio, s1 = partial_token_ratio.  Multiplications
// and maxima only, in exactly this association.
STRSIM_HD double wratio_rule(uint32_t cls, double r, double s0, double s1)
{
    if (cls == WRATIO_EMPTY) return 0.0;
    if (cls == WRATIO_NEAR) return wratio_max(r, s0 * 0.95);
    const double ps = cls == WRATIO_FAR8 ? 0.9 : 0.6;
    return wratio_max(wratio_max(r, s0 * ps), (s1 * 0.95) * ps);
}

// The rule of partial_token_set_ratio; p = partial_ratio(ab, ba).
STRSIM_HD double partial_token_set_score(const TokenSetRec &r, double p)
{
    if (r.flags & TOKEN_FLAG_ZERO) return 0.0;
    if (r.sl != 0u) return 1.0; // (a common token has a scalar value at least)
    return p;
}

// Four bytes of a source that starts `shift` bytes into the aligned dword lo (hi = the dword behind it, read only when shift != 0).
STRSIM_HD uint32_t wratio_funnel(uint32_t lo, uint32_t hi, uint32_t shift)
{
    return shift == 0u ? lo : (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * shift));
}

constexpr uint32_t TAKE_LANES = 8u; // lanes that copy one row

// Lane `sub` of TAKE_LANES copies its share of src[0, len) to dst.  The destination is written in aligned dwords (bytes up to the
// first and behind the last one), each from the one or two aligned source dwords that hold its bytes: every dword read holds a byte
// of the row, every byte written is the row's.
STRSIM_HD void take_copy(const uint8_t *src, uint8_t *dst, uint32_t len, uint32_t sub)
{
    uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    head = head < len ? head : len;
    if (sub < head) dst[sub] = src[sub];
    const uint32_t nd = (len - head) >> 2;
    const uint32_t shift = (uint32_t)((uintptr_t)(src + head) & 3u);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + head - shift);
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t k = sub; k < nd; k += TAKE_LANES) dw[k] = wratio_funnel(sw[k], shift != 0u ? sw[k + 1u] : 0u, shift);
    const uint32_t done = head + 4u * nd;
    if (sub < len - done) dst[done + sub] = src[done + sub];
}

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

constexpr int WRATIO_THREADS = 256;

// scalar values of n bytes of valid UTF-8 by one lane: whole aligned dwords inside the string, bytes at its ends
__device__ __forceinline__ uint32_t wratio_chars(const uint8_t *p, uint32_t n)
{
    uint32_t c = 0u, i = 0u;
    for (; i < n && ((uintptr_t)(p + i) & 3u) != 0u; ++i) c += (p[i] & 0xC0u) != 0x80u;
    for (; i + 4u <= n; i += 4u) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(p + i);
        c += 4u - (uint32_t)__popc((w >> 7) & ~(w >> 6) & 0x01010101u); // (a continuation byte is 10xxxxxx)
    }
    for (; i < n; ++i) c += (p[i] & 0xC0u) != 0x80u;
    return c;
}

// scalar values of a literal by the whole workgroup (s_acc zeroed by the caller behind a barrier)
__device__ __forceinline__ uint32_t wratio_chars_block(const uint8_t *p, uint32_t n, uint32_t *s_acc)
{
    uint32_t c = 0u;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) c += (p[i] & 0xC0u) != 0x80u;
    for (int d = 32; d >= 1; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d, 64);
    if ((threadIdx.x & 63u) == 0u && c != 0u) atomicAdd(s_acc, c);
    __syncthreads();
    return *s_acc;
}

// One pair per lane; rows_a / rows_b == 1: that side is a literal, counted once a workgroup.  cls[row] = the class, pos[row] = the
// row's position on its list (near: list_near, counted in st->rows[0]; far: list_far, st->rows[1]; both zeroed before the launch).
__global__ __launch_bounds__(WRATIO_THREADS) void k_wratio_classify(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rows_a,
                                                                    const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rows_b,
                                                                    uint64_t n, uint8_t *__restrict__ cls, uint32_t *__restrict__ pos,
                                                                    uint32_t *__restrict__ list_near, uint32_t *__restrict__ list_far, WratioStatus *st)
{
    __shared__ uint32_t s_lit[2];
    if (threadIdx.x < 2u) s_lit[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = row < n;
    uint32_t la, lb;
    if (rows_a == 1) la = wratio_chars_block(valA + offA[0], offA[1] - offA[0], &s_lit[0]);
    else {
        const uint32_t o = live ? offA[row] : 0u;
        la = live ? wratio_chars(valA + o, offA[row + 1] - o) : 0u;
    }
    if (rows_b == 1) lb = wratio_chars_block(valB + offB[0], offB[1] - offB[0], &s_lit[1]);
    else {
        const uint32_t o = live ? offB[row] : 0u;
        lb = live ? wratio_chars(valB + o, offB[row + 1] - o) : 0u;
    }
    const uint32_t c = live ? wratio_class(la, lb) : WRATIO_EMPTY;
    const uint32_t pn = wave_append(c == WRATIO_NEAR, (uint32_t)row, list_near, &st->rows[0]);
    const uint32_t pf = wave_append(c >= WRATIO_FAR8, (uint32_t)row, list_far, &st->rows[1]);
    if (live) {
        cls[row] = (uint8_t)c;
        pos[row] = c == WRATIO_NEAR ? pn : pf;
    }
}

// out_off[p + 1] = the bytes of row list[p] (out_off[0] = 0), p < m: the lengths the offset scan turns into the sub-column's offsets
__global__ __launch_bounds__(WRATIO_THREADS) void k_take_measure(const uint32_t *__restrict__ off, const uint32_t *__restrict__ list, uint32_t m,
                                                                 uint32_t *__restrict__ out_off)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) out_off[0] = 0u;
    if (p >= m) return;
    const uint32_t row = list[p];
    out_off[p + 1] = off[row + 1] - off[row];
}

// The values of row list[p] to out_val + out_off[p], TAKE_LANES lanes a row (take_copy).
__global__ __launch_bounds__(WRATIO_THREADS) void k_take_write(const uint32_t *__restrict__ off, const uint8_t *__restrict__ val,
                                                               const uint32_t *__restrict__ list, uint32_t m, const uint32_t *__restrict__ out_off,
                                                               uint8_t *__restrict__ out_val)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t p = t / TAKE_LANES;
    const uint32_t sub = (uint32_t)(t % TAKE_LANES);
    if (p >= m) return;
    const uint32_t row = list[p];
    const uint32_t s0 = off[row];
    take_copy(val + s0, out_val + out_off[p], off[row + 1] - s0, sub);
}

// out[row] = the rule of WRatio; out[row] holds r = indel(a, b) on entry.  near: s_near[pos] = token_ratio; far: s_far0[pos] =
// partial_ratio, s_far1[pos] = partial_token_ratio (pos: the row's place on its list).
__global__ __launch_bounds__(WRATIO_THREADS) void k_wratio_combine(const uint8_t *__restrict__ cls, const uint32_t *__restrict__ pos,
                                                                   const double *__restrict__ s_near, const double *__restrict__ s_far0,
                                                                   const double *__restrict__ s_far1, double *__restrict__ out, uint64_t n)
{
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint32_t c = cls[row], p = pos[row];
    double s0 = 0.0, s1 = 0.0;
    if (c == WRATIO_NEAR) s0 = s_near[p];
    else if (c != WRATIO_EMPTY) { s0 = s_far0[p]; s1 = s_far1[p]; }
    out[row] = wratio_rule(c, out[row], s0, s1);
}

// out[i] = max(x[i], y[i]) (out may be x or y)
__global__ __launch_bounds__(WRATIO_THREADS) void k_max_f64(const double *x, const double *y, double *out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = wratio_max(x[i], y[i]);
}

// out[row] = the rule of partial_token_set_ratio over the record and p[row] = partial_ratio(ab, ba) (out may be p)
__global__ __launch_bounds__(WRATIO_THREADS) void k_partial_token_set_epilogue(const TokenSetRec *__restrict__ rec, const double *p, double *out,
                                                                               uint64_t n)
{
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row < n) out[row] = partial_token_set_score(rec[row], p[row]);
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
