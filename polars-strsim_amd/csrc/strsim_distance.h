// strsim_distance.h -- bounded edit distances as integers: Levenshtein (measure 0) and optimal string alignment (measure 6),
// for strsim_distance_device / _host.
//
// d is the edit distance over Unicode scalar values (Levenshtein: insert, delete, substitute; OSA: plus the restricted swap of two
// adjacent characters of strsim_osa.h).  With a cutoff k (max_distance != STRSIM_DISTANCE_UNBOUNDED) a row's output is d when
// d <= k and k + 1 otherwise (rapidfuzz's score_cutoff convention).
//
// Two tiers, both finished in stream order:
//   k_dist_lane<TR, LIT>  one pair per lane, both strings ASCII and <= 64 bytes: the lane class, bit-planes and text walk of
//                         k_osa_lane; TR = 1 adds the transposition term (OSA), TR = 0 is Myers' step.  A pair whose lengths
//                         differ by more than k is k + 1 without the DP.  Every other row goes to a work list.
//   k_dist_wave<TR>       one pair per wave for the work list: any UTF-8, any length, the decode and pattern storage of k_osa_wave
//                         and its word step (osa_word_step).
//                         With a cutoff only the words 0..y of a column are advanced (the block cutoff of Myers 1999, section 4,
//                         as in edlib), y being the last word that may still hold a cell <= k (dist_column below).
#pragma once
#include <stdint.h>

#include "strsim_osa.h"

namespace strsim {

constexpr uint32_t DIST_UNBOUNDED = 0xFFFFFFFFu; // = STRSIM_DISTANCE_UNBOUNDED

// the output of a row: d, or k + 1 when d > k (never taken for k = DIST_UNBOUNDED: d < 2^32)
STRSIM_HD uint32_t dist_clamp(uint64_t d, uint32_t k) { return d > (uint64_t)k ? k + 1u : (uint32_t)d; }

// Length prefilter of both tiers: d >= | |a| - |b| |, so a pair whose lengths (in scalar values) differ by more than k is k + 1
// without the DP.
STRSIM_HD bool dist_length_cut(uint32_t la, uint32_t lb, uint32_t k) { return (la > lb ? la - lb : lb - la) > k; }

// What k_dist_lane does with a row (shared with the host harness): DIST_ROW_WAVE -- not both ASCII and <= 64 bytes, to the work
// list; DIST_ROW_CUT -- k + 1 by the length prefilter; DIST_ROW_RUN -- the lane DP; DIST_ROW_NONE -- past the end of the call.
// fits = both lengths <= OSA_LANE_MAX_BYTES (dist_lane_fits); ascii is only looked at (and only loaded) for a row that fits.
enum DistRow : uint32_t { DIST_ROW_NONE = 0, DIST_ROW_WAVE = 1, DIST_ROW_CUT = 2, DIST_ROW_RUN = 3 };
STRSIM_HD bool dist_lane_fits(uint32_t la, uint32_t lb) { return la <= OSA_LANE_MAX_BYTES && lb <= OSA_LANE_MAX_BYTES; }
STRSIM_HD uint32_t dist_lane_row(bool live, uint32_t la, uint32_t lb, bool ascii, uint32_t k)
{
    if (!live) return DIST_ROW_NONE;
    if (!dist_lane_fits(la, lb) || !ascii) return DIST_ROW_WAVE;
    return dist_length_cut(la, lb, k) ? DIST_ROW_CUT : DIST_ROW_RUN; // (ASCII: bytes are scalar values)
}

// One Levenshtein column on a single mask word (Myers 1999).
template <typename T>
STRSIM_HD void lev_step(T Eq, T &VP, T &VN)
{
    const T D0 = (((Eq & VP) + VP) ^ VP) | Eq | VN;
    const T HP = VN | ~(D0 | VP);
    const T HN = D0 & VP;
    const T X = (HP << 1) | (T)1;
    VP = (HN << 1) | ~(D0 | X);
    VN = D0 & X;
}

// Edit distance of an ASCII pattern against the text in wt: osa_lane_core with the step chosen by TR.
template <typename T, bool TR>
STRSIM_HD uint32_t dist_lane_core(const uint32_t (&wt)[16], uint32_t lt, uint32_t tmax, const uint32_t (&Plo)[7],
                                  const uint32_t (&Phi)[7], uint32_t lp)
{
    T VP = ~(T)0, VN = 0, D0p = 0, EQp = 0;
    unrolled_until<0, 64>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if ((uint32_t)j >= tmax) return false;
        if ((uint32_t)j < lt) {
            const T Eq = osa_eq<T>(Plo, Phi, wt[j >> 2], j & 3);
            if constexpr (TR) osa_step<T>(Eq, VP, VN, D0p, EQp);
            else lev_step<T>(Eq, VP, VN);
        }
        return true;
    });
    (void)D0p; (void)EQp;
    const T rows = lp >= 8 * sizeof(T) ? ~(T)0 : (((T)1 << lp) - (T)1);
    return lt + osa_popc((T)(VP & rows)) - osa_popc((T)(VN & rows));
}

// The state of one 64-row mask word of k_dist_wave: Myers' vertical deltas, the previous column's D0 and Eq (OSA), and the
// score of the word's bottom row (row 64 (w + 1), the padding rows of the last word included).
struct DistWord {
    uint64_t VP, VN, D0p, EQp, score;
};

// k_dist_wave scratch of one wave for patterns of up to m scalar values: the values (padded to whole words) and a DistWord per word
STRSIM_HD uint64_t dist_wave_slot_words(uint64_t m)
{
    const uint64_t words = (m + 63u) / 64u;
    return words * 64u + words * (sizeof(DistWord) / 4u);
}

// Words active before the first column: those with a row <= k (column 0 holds D[i][0] = i); all W without a cutoff.  -1: none.
STRSIM_HD int dist_first_y(uint32_t W, uint64_t m, uint64_t k, bool bounded)
{
    if (!bounded) return (int)W - 1;
    const uint64_t top = k < m ? k : m; // the last pattern row whose column-0 value is <= k
    return top == 0 ? -1 : (int)((top - 1) / 64u);
}

// One text column over the active words 0..y (y is updated).  c: the columns already done (D[0][c] = c, the top boundary row).
// eq(w): the match word of pattern word w against this column's character.  With a cutoff (bounded):
//   - word y + 1 is taken in when the bottom score of word y (of the boundary row for y = -1) in the previous column is <= k:
//     only then can a cell of word y + 1 be <= k in this column.  It starts as if every row were one
//     more than the row above (VP = ~0, VN = 0), counted from that score, with D0p = EQp = 0 (no transposition into it now);
//   - afterwards, while word y's bottom score is >= k + 64, every cell of it is > k (neighbouring rows differ by at most 1) and
//     y drops by one.
// Words beyond y keep stale state; computed cells are never below the true ones, and equal them wherever the true value is <= k.
template <bool TR, typename EqFn>
STRSIM_HD void dist_column(DistWord *st, int &y, uint32_t W, uint64_t k, uint64_t c, bool bounded, EqFn &&eq)
{
    if (bounded && y + 1 < (int)W) {
        const uint64_t above = y < 0 ? c : st[y].score;
        if (above <= k) {
            ++y;
            DistWord &n = st[y];
            n.VP = ~0ull; n.VN = 0ull; n.D0p = 0ull; n.EQp = 0ull;
            n.score = above + 64u;
        }
    }
    uint64_t add_c = 0ull, hp_c = 1ull, hn_c = 0ull, tr_c = 0ull;
    for (int w = 0; w <= y; ++w) {
        DistWord &s = st[w];
        osa_word_step<TR>(eq((uint32_t)w), s.VP, s.VN, s.D0p, s.EQp, add_c, hp_c, hn_c, tr_c);
        s.score = s.score + hp_c - hn_c;
    }
    if (bounded)
        while (y >= 0 && st[y].score >= k + 64u) --y;
}

// The result once the columns are done: d from the last column when every word is active, else > k.
STRSIM_HD uint64_t dist_final(const DistWord *st, int y, uint32_t W, uint64_t m, uint64_t nt, uint64_t k)
{
    if (y != (int)W - 1) return k + 1u;
    uint64_t up = 0u, dn = 0u;
    for (uint32_t w = 0; w < W; ++w) {
        const uint64_t r = m - 64u * w;
        const uint64_t rows = r >= 64u ? ~0ull : ((1ull << r) - 1ull);
        up += (uint64_t)osa_popc(st[w].VP & rows);
        dn += (uint64_t)osa_popc(st[w].VN & rows);
    }
    return nt + up - dn;
}

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

// One pair per lane (k_osa_lane's classes and text walk).  TR: 1 = OSA, 0 = Levenshtein.  LIT as k_osa_lane.  A row whose
// lengths differ by more than k is k + 1 without the DP, and a wave of such rows runs no columns.  Rows this kernel cannot take
// are appended to `worklist` (worklist_append of strsim_wave_util.h); the status block is zeroed before the launch.
template <bool TR, int LIT>
__global__ __launch_bounds__(256) void k_dist_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA,
                                                   const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t n,
                                                   uint32_t k, uint32_t *__restrict__ out, uint32_t *__restrict__ worklist,
                                                   DevStatus *st)
{
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = row < n;
    const uint64_t ia = (LIT == 1 || !live) ? 0 : row, ib = (LIT == 2 || !live) ? 0 : row;
    const uint32_t a0 = offA[ia], la = offA[ia + 1] - a0;
    const uint32_t b0 = offB[ib], lb = offB[ib + 1] - b0;
    const bool fits = live && dist_lane_fits(la, lb);
    const bool a_is_pat = LIT == 1 ? false : (LIT == 2 ? true : la >= lb);
    const uint8_t *pv = a_is_pat ? valA : valB, *tv = a_is_pat ? valB : valA;
    const uint32_t po = a_is_pat ? a0 : b0, to = a_is_pat ? b0 : a0;
    const uint32_t lp = a_is_pat ? la : lb, lt = a_is_pat ? lb : la;
    uint32_t wp[16] = {}, wt[16] = {};
    bool ascii = false;
    if (fits) {
        osa_load64(pv, po, lp, wp);
        osa_load64(tv, to, lt, wt);
        ascii = (osa_high_bits(wp) | osa_high_bits(wt)) == 0u;
    }
    const uint32_t cls = dist_lane_row(live, la, lb, ascii, k);
    worklist_append<false>(cls == DIST_ROW_WAVE, row, la, lb, worklist, st);
    if (cls == DIST_ROW_CUT) out[row] = k + 1u;
    const bool run = cls == DIST_ROW_RUN;
    if (__ballot(run) == 0ull) return;
    const uint32_t tmax = osa_wave_max(run ? lt : 0u);
    const uint32_t pmax = osa_wave_max(run ? lp : 0u);
    uint32_t Plo[7], Phi[7];
    osa_planes(wp, Plo, Phi, pmax > 32u);
    uint32_t d;
    if (pmax <= 32u) d = dist_lane_core<uint32_t, TR>(wt, run ? lt : 0u, tmax, Plo, Phi, lp);
    else d = dist_lane_core<uint64_t, TR>(wt, run ? lt : 0u, tmax, Plo, Phi, lp);
    if (run) out[row] = dist_clamp(d, k);
}

// One pair per wave (blockDim.x = 64) for the rows k_dist_lane put on the work list.  scratch: gridDim.x slots of slot_words
// words for patterns of more than OSA_WAVE_LDS_CPS values (nullptr when the call has none).
template <bool TR>
__global__ __launch_bounds__(64) void k_dist_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                  const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                                  uint32_t k, uint32_t *__restrict__ out, const uint32_t *__restrict__ worklist,
                                                  const DevStatus *st, uint32_t *scratch, uint64_t slot_words)
{
    __shared__ uint32_t s_pat[OSA_WAVE_LDS_CPS];
    __shared__ DistWord s_state[OSA_WAVE_LDS_CPS / 64u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = st->wave_rows;
    for (uint32_t r = blockIdx.x; r < count; r += gridDim.x) {
        const auto [row, pa, pb, na, nb, ca, cb] = wave_pair(offA, valA, rowsA, offB, valB, rowsB, worklist[r]);
        const bool a_is_pat = ca <= cb;
        const uint8_t *pp = a_is_pat ? pa : pb, *tp = a_is_pat ? pb : pa;
        const uint32_t pbytes = a_is_pat ? na : nb, tbytes = a_is_pat ? nb : na;
        const uint32_t m = a_is_pat ? ca : cb, nt = a_is_pat ? cb : ca;
        uint64_t d = nt;
        if (dist_length_cut(m, nt, k)) {
            d = (uint64_t)k + 1u;
        } else if (m != 0u) {
            const uint32_t W = (m + 63u) / 64u;
            const bool bounded = k < nt; // (d <= nt: a larger k cuts nothing)
            uint32_t *pat = s_pat;
            DistWord *state = s_state;
            if (m > OSA_WAVE_LDS_CPS) {
                pat = scratch + (uint64_t)blockIdx.x * slot_words;
                state = reinterpret_cast<DistWord *>(pat + (uint64_t)W * 64u);
            }
            wave_decode(pp, pbytes, pat, lane);
            for (uint32_t i = m + lane; i < W * 64u; i += 64u) pat[i] = 0xFFFFFFFFu;
            int y = dist_first_y(W, m, k, bounded);
            for (uint32_t w = lane; w < W; w += 64u) state[w] = DistWord{~0ull, 0ull, 0ull, 0ull, 64ull * (w + 1u)};
            __syncthreads();
            uint64_t c = 0u;
            const bool done = wave_each_char(tp, tbytes, lane, [&](uint32_t ch) {
                dist_column<TR>(state, y, W, k, c, bounded, [&](uint32_t w) { return (uint64_t)__ballot(pat[64u * w + lane] == ch); });
                ++c;
                return !(y < 0 && c > k); // false: no cell of this column is <= k (row 0 holds c), the pair is decided
            });
            d = done ? dist_final(state, y, W, m, nt, k) : (uint64_t)k + 1u;
            __syncthreads(); // (the next row overwrites pat / state)
        }
        if (lane == 0u) out[row] = dist_clamp(d, k);
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
