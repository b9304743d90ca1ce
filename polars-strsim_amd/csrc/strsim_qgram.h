// strsim_qgram.h -- q-gram similarity (strsim_qgram_device / _host): Jaccard, Sorensen-Dice, overlap and cosine over the
// contiguous q-tuples of Unicode scalar values, q = 1, 2 or 3.  It has no measure id: q and the mode do not fit strsim_pairs_device.
//
// G(s) is the multiset of the max(|s| - q + 1, 0) grams of s.  Multiset mode: na = |G(a)|, nb = |G(b)|, I = sum over the grams of
// min(count_a, count_b).  Set mode (STRSIM_QGRAM_SET): na, nb the numbers of distinct grams, I the number of grams in both.  Then
//   a == b bytewise -> 1.0;  na == 0 or nb == 0 -> 0.0;  else by kind
//   jaccard I / (na + nb - I)   sorensen_dice 2 I / (na + nb)   overlap I / min(na, nb)   cosine I / sqrt(na nb)
// (qgram_score).  With na, nb > 0 every formula gives exactly 1.0 for a == b by itself, so the byte compare is only made when both
// strings are shorter than q.  At q = 1 in multiset mode jaccard and sorensen_dice are measures 3 and 4, bit for bit.
//
// Two tiers, both finished in stream order:
//   k_qgram_lane<Q, SET>   one pair per lane, both strings ASCII and <= 64 bytes.  b is the pattern: seven bit-planes of one or two
//                          32-bit words (build_planes<7>), the width chosen per wave.  With E(c) the positions of b that hold c,
//                          the grams of b equal to the gram of a at i are E(a_i) & (E(a_i+1) >> 1) & (E(a_i+2) >> 2), cut to b's
//                          grams.  Multiset: every gram of a takes the lowest gram of b it equals that is still free (equal grams
//                          of b are interchangeable, so taking any free one is a maximum matching).  Set: a gram of a counts at its
//                          first occurrence -- the same mask against a's own planes, below i, is empty -- and is in the
//                          intersection when its mask against b is not; b's distinct grams are counted by the self-test over b.
//                          Every other row is appended to a work list.
//   k_qgram_wave<CAP>      one pair per wave for the work list: any UTF-8, any length.  One open-addressing table per pair over the
//                          grams of both strings: a 64-bit key (21 bits a scalar value) claimed by a compare-and-swap against
//                          QGRAM_EMPTY, and one count word whose halves count the gram in a and in b.  One pass over the slots
//                          gives I, and in set mode na and nb.  Up to CAP grams the table is in LDS, beyond in the context's
//                          scratch.
#pragma once
#include <math.h>
#include <stdint.h>

#include "strsim_indel.h"

namespace strsim {

constexpr int QGRAM_JACCARD = 0, QGRAM_SORENSEN_DICE = 1, QGRAM_OVERLAP = 2, QGRAM_COSINE = 3; // = STRSIM_QGRAM_*
constexpr uint32_t QGRAM_MAX_Q = 3u;
constexpr uint32_t QGRAM_LANE_MAX_BYTES = 64u;       // k_qgram_lane: both strings ASCII and at most this long
constexpr uint32_t QGRAM_WAVE_SMALL_GRAMS = 256u;    // k_qgram_wave<CAP>: the two table sizes held in LDS, in grams of both strings
constexpr uint32_t QGRAM_WAVE_LDS_GRAMS = 2048u;
constexpr uint64_t QGRAM_EMPTY = ~0ull;              // no key: a key has bit 63 clear

// rule 1 (same: a == b, which the caller tests only where both strings are shorter than q), rule 2, then the score by kind
STRSIM_HD double qgram_score(int kind, uint64_t isect, uint64_t na, uint64_t nb, bool same)
{
    if (same) return 1.0;
    if (na == 0 || nb == 0) return 0.0;
    switch (kind) {
    case QGRAM_JACCARD: return epilogue_jaccard(isect, na, nb);
    case QGRAM_SORENSEN_DICE: return epilogue_sorensen_dice(isect, na, nb);
    case QGRAM_OVERLAP: return (double)isect / (double)(na < nb ? na : nb);
    default: return (double)isect / sqrt((double)(na * nb));
    }
}

STRSIM_HD uint32_t qgram_count(uint32_t len, uint32_t q) { return len >= q ? len - q + 1u : 0u; }

// ---- the lane core ----

template <typename T>
STRSIM_HD T qgram_low(uint32_t k)
{
    return k >= 8u * sizeof(T) ? ~(T)0 : (T)(((T)1 << k) - (T)1);
}

// E(c) for byte `byte` (0..3, static) of dword w over the pattern's planes: bytes 0..31 in Plo, 32..63 in Phi; `valid` is 0 or ~0
template <typename T>
STRSIM_HD T qgram_eq(const uint32_t (&Plo)[7], const uint32_t (&Phi)[7], uint32_t valid, uint32_t w, int byte)
{
    const uint32_t lo = eq_mask<7>(Plo, valid, w, byte);
    if constexpr (sizeof(T) == 4) {
        (void)Phi;
        return lo;
    } else {
        return ((uint64_t)eq_mask<7>(Phi, valid, w, byte) << 32) | lo;
    }
}

// The step of every walk, in two halves.  With E the positions of the pattern that hold the text's byte j: gram(E) is the set of
// pattern grams equal to the text gram that byte j completes (the one that starts at j - Q + 1), and push(E) then takes E into the
// two masks behind it.  Before the text's first gram is complete the masks behind are empty, and so is gram(E).
template <typename T, int Q>
struct QgramGrams {
    T acc1 = 0, acc2 = 0;
    STRSIM_HD T gram(T E) const { return Q == 1 ? E : (Q == 2 ? (T)(acc1 & (E >> 1)) : (T)(acc2 & (E >> 2))); }
    STRSIM_HD void push(T E)
    {
        if constexpr (Q == 3) acc2 = acc1 & (E >> 1);
        if constexpr (Q >= 2) acc1 = E;
    }
};

// The greedy of the multiset intersection: the text gram whose equal pattern grams are M takes the lowest of them that is still
// free (M is already cut to the pattern's grams) -> 1 when it found one.
template <typename T>
STRSIM_HD uint32_t qgram_take(T M, T &used)
{
    const T m = M & ~used;
    used |= m & ((T)0 - m);
    return m != 0 ? 1u : 0u;
}

enum QgramWalk : int {
    QGRAM_GREEDY = 0, // -> the number of text grams that found a free equal gram among the pattern's first gp
    QGRAM_HIT = 1,    // -> bit i: text gram i equals one of the pattern's first gp grams
    QGRAM_SEEN = 2    // -> bit i: text gram i equals a pattern gram below i (the pattern is the text itself: not a first occurrence)
};

// The grams of the text wt (lt <= 8 sizeof(T) bytes, zero behind them) against the planes of the pattern.  Bytes at or beyond tmax
// are not looked at (wave-uniform, >= lt); the match mask of a byte at or beyond lt is empty, so that a gram which reaches past
// the text equals nothing: padding forms no gram, and a NUL inside a string is a character like any other.  The gram that starts
// at i is complete with byte j = i + Q - 1.  No branch in here depends on the lane.
template <typename T, int Q, int MODE>
STRSIM_HD uint64_t qgram_walk(const uint32_t (&wt)[16], uint32_t lt, uint32_t tmax, const uint32_t (&Plo)[7], const uint32_t (&Phi)[7],
                              uint32_t gp)
{
    const uint32_t vm[2] = {low_ones(lt), low_ones(lt > 32u ? lt - 32u : 0u)};
    const T rows = qgram_low<T>(gp);
    QgramGrams<T, Q> grams;
    T used = 0;
    uint64_t res = 0ull;
    unrolled_until<0, (int)(8 * sizeof(T))>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if ((uint32_t)j >= tmax) return false;
        const T E = qgram_eq<T>(Plo, Phi, bit_fill(vm[j >> 5], j & 31), wt[j >> 2], j & 3);
        if constexpr (j >= Q - 1) {
            constexpr int i = j - (Q - 1);
            T M = grams.gram(E);
            if constexpr (MODE == QGRAM_GREEDY) {
                res += qgram_take<T>(M & rows, used);
            } else {
                M &= MODE == QGRAM_HIT ? rows : qgram_low<T>((uint32_t)i);
                res |= M != 0 ? (1ull << i) : 0ull;
            }
        }
        grams.push(E);
        return true;
    });
    return res;
}

struct QgramCounts {
    uint32_t isect, na, nb;
};

// One pair: a (la bytes, amax the wave's longest a) is the text, b (lb bytes, bmax) the pattern; T holds max(la, lb) bits.
template <typename T, int Q, bool SET>
STRSIM_HD QgramCounts qgram_lane_pair(const uint32_t (&wa)[16], uint32_t la, uint32_t amax, const uint32_t (&wb)[16], uint32_t lb,
                                      uint32_t bmax)
{
    constexpr bool HI = sizeof(T) == 8;
    const uint32_t ga = qgram_count(la, Q), gb = qgram_count(lb, Q);
    uint32_t Plo[7], Phi[7];
    osa_planes(wb, Plo, Phi, HI);
    if constexpr (!SET) {
        (void)bmax;
        return QgramCounts{(uint32_t)qgram_walk<T, Q, QGRAM_GREEDY>(wa, la, amax, Plo, Phi, gb), ga, gb};
    } else {
        const uint64_t hit = qgram_walk<T, Q, QGRAM_HIT>(wa, la, amax, Plo, Phi, gb);
        const uint64_t seen_b = qgram_walk<T, Q, QGRAM_SEEN>(wb, lb, bmax, Plo, Phi, 0u);
        osa_planes(wa, Plo, Phi, HI);
        const uint64_t seen_a = qgram_walk<T, Q, QGRAM_SEEN>(wa, la, amax, Plo, Phi, 0u);
        const uint64_t first_a = ~seen_a & qgram_low<uint64_t>(ga), first_b = ~seen_b & qgram_low<uint64_t>(gb);
        return QgramCounts{osa_popc((uint64_t)(first_a & hit)), osa_popc(first_a), osa_popc(first_b)};
    }
}

// ---- the table rules ----

// the key of the gram v0 [v1 [v2]] (scalar values, each below 2^21; the ones a shorter gram does not have are 0)
STRSIM_HD uint64_t qgram_key(uint32_t v0, uint32_t v1, uint32_t v2) { return (uint64_t)v0 | ((uint64_t)v1 << 21) | ((uint64_t)v2 << 42); }

// slots of the table of a pair with `grams` grams in both strings together: a power of two, load at most 1/2
STRSIM_HD uint64_t qgram_table_slots(uint64_t grams)
{
    uint64_t t = 64u;
    while (t < 2u * grams) t <<= 1;
    return t;
}

STRSIM_HD uint32_t qgram_hash(uint64_t key, uint32_t mask)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// The slot of `key` in keys[0 .. mask]: linear probing from its hash, an empty slot claimed by cas(p, expected, desired) -> the
// value found at p.  At most mask + 1 probes; with load <= 1/2 an empty slot or the key turns up before that.  Nothing waits for
// another claimant: a probe that loses its slot to another key moves on, one that loses it to the same key shares it.
template <class Cas>
STRSIM_HD uint32_t qgram_claim(uint64_t *keys, uint32_t mask, uint64_t key, Cas &&cas)
{
    uint32_t s = qgram_hash(key, mask);
    for (uint32_t probe = 0u; probe < mask; ++probe) {
        const uint64_t found = cas(keys + s, QGRAM_EMPTY, key);
        if (found == QGRAM_EMPTY || found == key) break;
        s = (s + 1u) & mask;
    }
    return s;
}

// A slot's count word C (uint32_t in LDS, uint64_t in scratch): the low half counts the gram in a, the high half in b.
template <typename C>
STRSIM_HD C qgram_count_one(int side) { return side ? (C)((C)1 << (4 * sizeof(C))) : (C)1; }

// what one slot adds to I, and in set mode to na and nb
template <typename C, bool SET>
STRSIM_HD void qgram_tally(C cnt, uint32_t &isect, uint32_t &da, uint32_t &db)
{
    const C half = (C)(((C)1 << (4 * sizeof(C))) - (C)1);
    const C ca = cnt & half, cb = cnt >> (4 * sizeof(C));
    if constexpr (SET) {
        isect += (ca != 0 && cb != 0) ? 1u : 0u;
        da += ca != 0 ? 1u : 0u;
        db += cb != 0 ? 1u : 0u;
    } else {
        isect += (uint32_t)(ca < cb ? ca : cb);
    }
}

// Words of scratch of one k_qgram_wave wave for pairs of up to `grams` grams and `values` scalar values a string: 64-bit keys,
// 64-bit counts, the values of one string (an even number of words: the 64-bit arrays come first).
STRSIM_HD uint64_t qgram_wave_slot_words(uint64_t grams, uint64_t values)
{
    return 4u * qgram_table_slots(grams) + ((values + 5u) & ~(uint64_t)1);
}

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

// One pair per lane.  A side with one row is a literal, read as row 0 by every lane.  Rows this kernel cannot take are appended to
// `worklist`: st->wave_rows counts them, st->max_len and st->pad1[0] bound the shorter and the longer string of a row (bytes).
// The status block is zeroed before the launch.
template <int Q, bool SET>
__global__ __launch_bounds__(256) void k_qgram_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                    const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                                    uint64_t n, int kind, double *__restrict__ out, uint32_t *__restrict__ worklist,
                                                    DevStatus *st)
{
    const auto [row, live, a0, la, b0, lb] = lane_row(offA, offB, n, rowsA == 1, rowsB == 1);
    const bool fits = live && la <= QGRAM_LANE_MAX_BYTES && lb <= QGRAM_LANE_MAX_BYTES;
    // a lane that does not fit loads nothing and has no gram
    const uint32_t lar = fits ? la : 0u, lbr = fits ? lb : 0u;
    uint32_t wa[16], wb[16];
    osa_load64(valA, a0, lar, wa);
    osa_load64(valB, b0, lbr, wb);
    // (eq_mask compares seven bits: a non-ASCII lane computes something harmless and is not written)
    const bool ok = fits && (osa_high_bits(wa) | osa_high_bits(wb)) == 0u;
    worklist_append<true>(live && !ok, row, la, lb, worklist, st); // rows for k_qgram_wave
    if (__ballot(ok) == 0ull) return;
    const bool wide = __ballot(lar > 32u || lbr > 32u) != 0ull;
    const uint32_t amax = indel_wave_max(lar), bmax = SET ? indel_wave_max(lbr) : 0u;
    const QgramCounts c = wide ? qgram_lane_pair<uint64_t, Q, SET>(wa, lar, amax, wb, lbr, bmax)
                               : qgram_lane_pair<uint32_t, Q, SET>(wa, lar, amax, wb, lbr, bmax);
    // both shorter than q (at most two bytes, the rest of the dword is zero)
    const bool same = la < (uint32_t)Q && lb < (uint32_t)Q && la == lb && wa[0] == wb[0];
    if (ok) out[row] = qgram_score(kind, c.isect, c.na, c.nb, same);
}

__device__ __forceinline__ uint32_t qgram_wave_sum(uint32_t v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
    return v;
}

// The g grams of the string whose scalar values are in vals, counted into the table as side `side`.
template <typename C, int Q>
__device__ __forceinline__ void qgram_wave_insert(const uint32_t *vals, uint32_t g, int side, uint64_t *keys, C *cnt, uint32_t mask,
                                                  uint32_t lane)
{
    for (uint32_t i = lane; i < g; i += 64u) {
        const uint64_t key = qgram_key(vals[i], Q >= 2 ? vals[i + (Q >= 2 ? 1 : 0)] : 0u, Q >= 3 ? vals[i + (Q >= 3 ? 2 : 0)] : 0u);
        const uint32_t s = qgram_claim(keys, mask, key, [](uint64_t *p, uint64_t expected, uint64_t desired) {
            return (uint64_t)atomicCAS(reinterpret_cast<unsigned long long *>(p), (unsigned long long)expected, (unsigned long long)desired);
        });
        if constexpr (sizeof(C) == 4) atomicAdd(reinterpret_cast<unsigned int *>(cnt + s), (unsigned int)qgram_count_one<C>(side));
        else atomicAdd(reinterpret_cast<unsigned long long *>(cnt + s), (unsigned long long)qgram_count_one<C>(side));
    }
}

// One pair through a table of `slots` slots (keys, cnt), with room for the values of one string in vals -> I, na, nb, the same in
// every lane.  ga, gb > 0.
template <typename C, int Q, bool SET>
__device__ __forceinline__ QgramCounts qgram_wave_table(const WavePair &p, uint32_t ga, uint32_t gb, uint64_t *keys, C *cnt, uint32_t *vals,
                                                        uint32_t slots, uint32_t lane)
{
    // (the table is written and read with atomic operations throughout: in scratch the compare-and-swaps and the adds are made in
    // the L2 cache, which a plain load through the L1 cache need not see)
    for (uint32_t s = lane; s < slots; s += 64u) {
        __hip_atomic_store(keys + s, QGRAM_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(cnt + s, (C)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    wave_decode(p.pa, p.na, vals, lane);
    __syncthreads();
    qgram_wave_insert<C, Q>(vals, ga, 0, keys, cnt, slots - 1u, lane);
    __syncthreads();
    wave_decode(p.pb, p.nb, vals, lane);
    __syncthreads();
    qgram_wave_insert<C, Q>(vals, gb, 1, keys, cnt, slots - 1u, lane);
    __syncthreads();
    uint32_t isect = 0u, da = 0u, db = 0u;
    for (uint32_t s = lane; s < slots; s += 64u)
        qgram_tally<C, SET>(__hip_atomic_load(cnt + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), isect, da, db);
    isect = qgram_wave_sum(isect);
    if constexpr (SET) {
        da = qgram_wave_sum(da);
        db = qgram_wave_sum(db);
    } else {
        da = ga;
        db = gb;
    }
    __syncthreads(); // (the next row overwrites the table)
    return QgramCounts{isect, da, db};
}

// One pair per wave (blockDim.x = 64) for the rows k_qgram_lane put on the work list (st->wave_rows of them).  Pairs of up to CAP
// grams use the table in LDS; scratch: gridDim.x slots of slot_words words for the others (nullptr when the call has none), each
// laid out for `scratch_slots` table slots.
template <uint32_t CAP, int Q, bool SET>
__global__ __launch_bounds__(64) void k_qgram_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                   const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                                   int kind, double *__restrict__ out, const uint32_t *__restrict__ worklist,
                                                   const DevStatus *st, uint32_t *scratch, uint64_t slot_words, uint64_t scratch_slots)
{
    __shared__ uint64_t s_keys[2u * CAP];
    __shared__ uint32_t s_cnt[2u * CAP];
    __shared__ uint32_t s_vals[CAP + 4u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = st->wave_rows;
    for (uint32_t r = blockIdx.x; r < count; r += gridDim.x) {
        const WavePair p = wave_pair(offA, valA, rowsA, offB, valB, rowsB, worklist[r]);
        const uint32_t ga = qgram_count(p.ca, Q), gb = qgram_count(p.cb, Q);
        QgramCounts c{0u, ga, gb};
        bool same = false;
        if (ga == 0u || gb == 0u) {
            // rule 1 where the formulas cannot give it: both strings shorter than q
            if (ga == 0u && gb == 0u && p.na == p.nb) {
                bool differ = false;
                for (uint32_t i = lane; i < p.na; i += 64u) differ = differ || p.pa[i] != p.pb[i];
                same = __ballot(differ) == 0ull;
            }
        } else if (ga + gb <= CAP) {
            // (a string has at most CAP - 1 grams here, so CAP + 1 values)
            c = qgram_wave_table<uint32_t, Q, SET>(p, ga, gb, s_keys, s_cnt, s_vals, (uint32_t)qgram_table_slots((uint64_t)ga + gb), lane);
        } else {
            uint64_t *keys = reinterpret_cast<uint64_t *>(scratch + (uint64_t)blockIdx.x * slot_words);
            uint64_t *cnt = keys + scratch_slots;
            uint32_t *vals = reinterpret_cast<uint32_t *>(cnt + scratch_slots);
            c = qgram_wave_table<uint64_t, Q, SET>(p, ga, gb, keys, cnt, vals, (uint32_t)qgram_table_slots((uint64_t)ga + gb), lane);
        }
        if (lane == 0u) out[p.row] = qgram_score(kind, c.isect, c.na, c.nb, same);
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
