// strsim_wave_util.h -- what the two-pass measures' kernels share on the device (strsim_osa.h, strsim_distance.h, strsim_indel.h,
// strsim_partial.h, strsim_token.h, strsim_wratio.h): a lane kernel takes the rows it can and appends the others to a work list, a
// wave kernel then takes one listed pair per wave.
//   lane_row, lane_pick                             the lane kernel's row (offsets, lengths) and its choice of pattern and text
//   wave_append, worklist_append                    the lane kernel's append of a row to the list (one atomic a wave)
//   osa_is_start, osa_decode_at, osa_count_chars    UTF-8 by the wave, 64 bytes at a time
//   wave_pair, wave_decode, wave_each_char          the wave kernel's pair, its pattern as scalar values, its text column by column
//   wave_stage, wave_pattern                        the wave kernel's pattern and text, where pattern and state live, the padded decode
// None of them holds a barrier: a kernel that stores through wave_decode and reads another lane's value puts its own
// __syncthreads() between the two.  (DevStatus: strsim_kernels.h, included before this header.)
#pragma once
#include <stdint.h>
#include <type_traits>

namespace strsim {

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)

__device__ __forceinline__ uint32_t osa_wave_max(uint32_t v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, s, 64);
        v = o > v ? o : v;
    }
    return v;
}

// ---- the lane kernel's side ----

// The row of a lane (blockDim.x rows a block): whether it is one of the call's n, and where its two strings start and how many bytes
// they have.  lit_a / lit_b: that side is a literal, row 0 for every lane (constants in the LIT kernels); a lane past the end reads
// row 0 of both sides.
struct LaneRow {
    uint64_t row;
    bool live;
    uint32_t a0, la, b0, lb;
};
__device__ __forceinline__ LaneRow lane_row(const uint32_t *__restrict__ offA, const uint32_t *__restrict__ offB, uint64_t n, bool lit_a,
                                            bool lit_b)
{
    LaneRow r;
    r.row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    r.live = r.row < n;
    const uint64_t ia = (lit_a || !r.live) ? 0 : r.row, ib = (lit_b || !r.live) ? 0 : r.row;
    r.a0 = offA[ia];
    r.la = offA[ia + 1] - r.a0;
    r.b0 = offB[ib];
    r.lb = offB[ib + 1] - r.b0;
    return r;
}

// Pattern and text of a lane's row.  LIT: 0 = row against row, the longer string is the pattern and the shorter one the text (fewer
// columns); 1 = a is a literal, 2 = b is: the literal is the text -- the same bytes in every lane, read through a wave-uniform
// address -- and the row string the pattern.  pv / tv: the value columns, po / to: the offsets, lp / lt: the byte lengths.
struct LanePick {
    bool a_is_pat;
    const uint8_t *pv, *tv;
    uint32_t po, to, lp, lt;
};
template <int LIT>
__device__ __forceinline__ LanePick lane_pick(const uint8_t *__restrict__ valA, const uint8_t *__restrict__ valB, const LaneRow &r)
{
    LanePick p;
    p.a_is_pat = LIT == 1 ? false : (LIT == 2 ? true : r.la >= r.lb);
    p.pv = p.a_is_pat ? valA : valB;
    p.tv = p.a_is_pat ? valB : valA;
    p.po = p.a_is_pat ? r.a0 : r.b0;
    p.to = p.a_is_pat ? r.b0 : r.a0;
    p.lp = p.a_is_pat ? r.la : r.lb;
    p.lt = p.a_is_pat ? r.lb : r.la;
    return p;
}

// Wave-aggregated append of the lanes with `take` to a work list: the first of them adds their number to *count, each stores its
// row at its rank behind that base.  Returns where the lane's row went (0 in a wave without any).
__device__ __forceinline__ uint32_t wave_append(bool take, uint32_t row, uint32_t *__restrict__ list, uint32_t *count)
{
    const uint64_t sm = __ballot(take);
    if (sm == 0ull) return 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t first = (uint32_t)__ffsll((unsigned long long)sm) - 1u;
    uint32_t base = 0u;
    if (lane == first) base = atomicAdd(count, (uint32_t)__popcll(sm));
    base = (uint32_t)__shfl((int)base, (int)first, 64);
    const uint32_t pos = base + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull));
    if (take) list[pos] = row;
    return pos;
}

// The same for a two-pass call's status block: st->wave_rows counts the rows, st->max_len bounds their patterns (the smaller of
// the two byte lengths) and, with HAY, st->pad1[0] their haystacks (the larger); the same lane makes all three atomics.  The block
// is zeroed before the launch.
template <bool HAY>
__device__ __forceinline__ void worklist_append(bool slow, uint64_t row, uint32_t la, uint32_t lb, uint32_t *__restrict__ worklist,
                                                DevStatus *st)
{
    const uint64_t sm = __ballot(slow);
    if (sm) {
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t first = (uint32_t)__ffsll((unsigned long long)sm) - 1u;
        const uint32_t bound = osa_wave_max(slow ? (la < lb ? la : lb) : 0u);
        uint32_t hbound = 0u;
        if constexpr (HAY) hbound = osa_wave_max(slow ? (la < lb ? lb : la) : 0u);
        uint32_t base = 0u;
        if (lane == first) {
            base = atomicAdd(&st->wave_rows, (uint32_t)__popcll(sm));
            atomicMax(&st->max_len, bound);
            if constexpr (HAY) atomicMax(&st->pad1[0], hbound);
        }
        base = (uint32_t)__shfl((int)base, (int)first, 64);
        if (slow) worklist[base + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull))] = (uint32_t)row;
    }
}

// ---- UTF-8 by the wave ----

// Decode the UTF-8 character that starts at p[i] (i < len; bytes past len are not read).
__device__ __forceinline__ uint32_t osa_decode_at(const uint8_t *__restrict__ p, uint32_t i, uint32_t len)
{
    const uint32_t b0 = p[i];
    auto cont = [&](uint32_t k) { return i + k < len ? (uint32_t)(p[i + k] & 0x3Fu) : 0u; };
    if (b0 < 0x80u) return b0;
    if (b0 < 0xE0u) return ((b0 & 0x1Fu) << 6) | cont(1);
    if (b0 < 0xF0u) return ((b0 & 0x0Fu) << 12) | (cont(1) << 6) | cont(2);
    return ((b0 & 0x07u) << 18) | (cont(1) << 12) | (cont(2) << 6) | cont(3);
}

__device__ __forceinline__ bool osa_is_start(const uint8_t *__restrict__ p, uint32_t i, uint32_t len)
{
    return i < len && (p[i] & 0xC0u) != 0x80u;
}

// scalar values of p[0, len), counted by the wave
__device__ __forceinline__ uint32_t osa_count_chars(const uint8_t *__restrict__ p, uint32_t len)
{
    uint32_t c = 0u;
    for (uint32_t base = 0u; base < len; base += 64u) c += (uint32_t)__popcll(__ballot(osa_is_start(p, base + (threadIdx.x & 63u), len)));
    return c;
}

// ---- the wave kernel's side ----

// The pair of work-list entry `row` (a side of one row is a literal): the two strings, their bytes (na, nb) and their scalar
// values (ca, cb).
struct WavePair {
    uint32_t row;
    const uint8_t *pa, *pb;
    uint32_t na, nb, ca, cb;
};
__device__ __forceinline__ WavePair wave_pair(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                              const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                              uint32_t row)
{
    WavePair p;
    p.row = row;
    const uint64_t ia = rowsA == 1 ? 0 : row, ib = rowsB == 1 ? 0 : row;
    p.pa = valA + offA[ia];
    p.pb = valB + offB[ib];
    p.na = offA[ia + 1] - offA[ia];
    p.nb = offB[ib + 1] - offB[ib];
    p.ca = osa_count_chars(p.pa, p.na);
    p.cb = osa_count_chars(p.pb, p.nb);
    return p;
}

// scalar values of p[0, bytes) into dst[0 ..), in order, by the wave
__device__ __forceinline__ void wave_decode(const uint8_t *__restrict__ p, uint32_t bytes, uint32_t *dst, uint32_t lane)
{
    uint32_t pos = 0u;
    for (uint32_t base = 0u; base < bytes; base += 64u) {
        const bool s = osa_is_start(p, base + lane, bytes);
        const uint64_t sm = __ballot(s);
        if (s) dst[pos + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull))] = osa_decode_at(p, base + lane, bytes);
        pos += (uint32_t)__popcll(sm);
    }
}

// Pattern and text of a wave kernel's pair -- the string with fewer scalar values is the pattern (m values, W words of 64), the
// other the text (nt values) -- and where the pattern's values and the State words behind them live: s_pat / s_state (LDS) for
// patterns of up to lds_cps values, else the wave's slot of `scratch` (slot_words words a wave, the state behind W whole words of
// values).  Nothing is loaded or stored here.
template <typename State>
struct WaveStage {
    uint32_t m, nt, W;
    const uint8_t *pp, *tp;
    uint32_t pbytes, tbytes;
    uint32_t *pat;
    State *state;
};
template <typename State>
__device__ __forceinline__ WaveStage<State> wave_stage(const WavePair &p, uint32_t *s_pat, State *s_state, uint32_t lds_cps,
                                                       uint32_t *scratch, uint64_t slot_words)
{
    const bool a_is_pat = p.ca <= p.cb;
    WaveStage<State> s;
    s.pp = a_is_pat ? p.pa : p.pb;
    s.tp = a_is_pat ? p.pb : p.pa;
    s.pbytes = a_is_pat ? p.na : p.nb;
    s.tbytes = a_is_pat ? p.nb : p.na;
    s.m = a_is_pat ? p.ca : p.cb;
    s.nt = a_is_pat ? p.cb : p.ca;
    s.W = (s.m + 63u) / 64u;
    s.pat = s_pat;
    s.state = s_state;
    if (s.m > lds_cps) {
        s.pat = scratch + (uint64_t)blockIdx.x * slot_words;
        s.state = reinterpret_cast<State *>(s.pat + (uint64_t)s.W * 64u);
    }
    return s;
}

// The pattern's m scalar values into pat, padded to `words` whole words of 64 with values that never match (no scalar value is
// 0xFFFFFFFF).  The barrier before another lane's value is read is the kernel's.
__device__ __forceinline__ void wave_pattern(const uint8_t *__restrict__ pp, uint32_t pbytes, uint32_t m, uint32_t words, uint32_t *pat,
                                             uint32_t lane)
{
    wave_decode(pp, pbytes, pat, lane);
    for (uint32_t i = m + lane; i < words * 64u; i += 64u) pat[i] = 0xFFFFFFFFu;
}

// f(ch) once per scalar value of p[0, bytes), in order, ch wave-uniform: 64 bytes are decoded at a time, one by each lane, and the
// values are handed round.  An f that returns bool ends the walk by returning false; the result tells whether it reached the end.
template <typename F>
__device__ __forceinline__ bool wave_each_char(const uint8_t *__restrict__ p, uint32_t bytes, uint32_t lane, F &&f)
{
    bool go = true;
    for (uint32_t base = 0u; base < bytes && go; base += 64u) {
        const bool s = osa_is_start(p, base + lane, bytes);
        const uint32_t cv = s ? osa_decode_at(p, base + lane, bytes) : 0u;
        uint64_t sm = __ballot(s);
        while (sm) {
            const int src = __ffsll((unsigned long long)sm) - 1;
            sm &= sm - 1ull;
            const uint32_t ch = (uint32_t)__shfl((int)cv, src, 64);
            if constexpr (std::is_void<decltype(f(ch))>::value) {
                f(ch);
            } else if (!f(ch)) {
                go = false;
                break;
            }
        }
    }
    return go;
}

#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
