// strsim_distance.h -- the edit-distance kernels: Levenshtein (measure 0) and optimal string alignment (measure 6) as bounded
// integers, for strsim_distance_device / _host, and the OSA similarity of strsim_pairs_device (section 11).
//
// d is the edit distance over Unicode scalar values (Levenshtein: insert, delete, substitute; OSA: plus the restricted swap of two
// adjacent characters of strsim_osa.h).  With a cutoff k (max_distance != STRSIM_DISTANCE_UNBOUNDED) a row's output is d when
// d <= k and k + 1 otherwise (rapidfuzz's score_cutoff convention).  The similarity is epilogue_osa of the unbounded d.
//
// Two tiers, both finished in stream order:
//   k_dist_lane<TR, LIT, OUT>  one pair per lane, both strings ASCII and <= 64 bytes; the pattern in seven bit-planes of 32 or 64
//                         bits (eq_mask of strsim_lane_core.h), the text walked byte by byte from registers.  TR = 1 adds the
//                         transposition term (OSA), TR = 0 is Myers' step.  A pair whose lengths differ by more than k is k + 1
//                         without the DP.  Every other row is appended to a work list (worklist_append of strsim_wave_util.h).
//   k_dist_wave<TR, OUT>  one pair per wave for the work list: any UTF-8, any length.  Both strings are decoded to scalar values;
//                         the shorter (in scalar values) is the pattern, held in LDS up to OSA_WAVE_LDS_CPS values and in the
//                         context's scratch above that (wave_stage of strsim_wave_util.h).  The match words of a text character
//                         are built 64 pattern values at a time by a compare and a ballot; the words are then advanced one after
//                         the other with the four carries between them (osa_word_step).
//                         With a cutoff only the words 0..y of a column are advanced (the block cutoff of Myers 1999, section 4,
//                         as in edlib), y being the last word that may still hold a cell <= k (dist_column below).
// OUT = uint32_t is the distance.  OUT = double is the similarity, instantiated for TR = 1 alone: k is DIST_UNBOUNDED at compile
// time, so the length cut, the clamp and the block cutoff's bookkeeping are compiled out.
#pragma once
#include <stdint.h>
#include <type_traits>

#include "strsim_osa.h"

namespace strsim {

constexpr uint32_t DIST_UNBOUNDED = 0xFFFFFFFFu; // = STRSIM_DISTANCE_UNBOUNDED

// the output of a row: d, or k + 1 when d > k (never taken for k = DIST_UNBOUNDED: d < 2^32)
STRSIM_HD uint32_t dist_clamp(uint64_t d, uint32_t k) { return d > (uint64_t)k ? k + 1u : (uint32_t)d; }

// what both tiers write for a pair of la and lb scalar values: the clamped distance, or as a double the similarity (k: none)
template <typename OUT>
STRSIM_HD OUT dist_result(uint64_t d, uint64_t la, uint64_t lb, uint32_t k)
{
    if constexpr (std::is_same<OUT, double>::value) return epilogue_osa(d, la, lb);
    else return dist_clamp(d, k);
}

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

// Edit distance of an ASCII pattern (lp <= 32 for T = uint32_t, <= 64 for uint64_t; planes from build_planes<7>) against the
// text in wt (lt <= 64 bytes), the step chosen by TR.  Columns tmax and beyond are not run (lane-uniform, >= lt); columns
// lt .. tmax-1 leave the state alone.
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
// The same without the score, for the similarity (never a cutoff): 32 bytes a word, which keeps the 16-byte halves of every word
// aligned -- in an array of DistWord those of every second word are not, and the wave kernel's loads and stores of them are slow.
struct DistWordFree {
    uint64_t VP, VN, D0p, EQp;
};
template <typename Word>
constexpr bool dist_scored = std::is_same<Word, DistWord>::value;

// word w before the first column
template <typename Word>
STRSIM_HD Word dist_word_start(uint32_t w)
{
    if constexpr (dist_scored<Word>) return Word{~0ull, 0ull, 0ull, 0ull, 64ull * (w + 1u)};
    else return Word{~0ull, 0ull, 0ull, 0ull};
}

// k_dist_wave scratch of one wave for patterns of up to m scalar values: the values (padded to whole words) and a DistWord per word
// (which holds the similarity's DistWordFree words as well)
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
// Words without a score (DistWordFree: never bounded, y = W - 1 throughout) leave the scores and the moves of y out of the code.
template <bool TR, typename Word, typename EqFn>
STRSIM_HD void dist_column(Word *st, int &y, uint32_t W, uint64_t k, uint64_t c, bool bounded, EqFn &&eq)
{
    constexpr bool SCORED = dist_scored<Word>;
    if constexpr (SCORED) {
        if (bounded && y + 1 < (int)W) {
            const uint64_t above = y < 0 ? c : st[y].score;
            if (above <= k) {
                ++y;
                DistWord &n = st[y];
                n.VP = ~0ull; n.VN = 0ull; n.D0p = 0ull; n.EQp = 0ull;
                n.score = above + 64u;
            }
        }
    }
    uint64_t add_c = 0ull, hp_c = 1ull, hn_c = 0ull, tr_c = 0ull;
    for (int w = 0; w <= y; ++w) {
        Word &s = st[w];
        osa_word_step<TR>(eq((uint32_t)w), s.VP, s.VN, s.D0p, s.EQp, add_c, hp_c, hn_c, tr_c);
        if constexpr (SCORED) s.score = s.score + hp_c - hn_c;
    }
    if constexpr (SCORED) {
        if (bounded)
            while (y >= 0 && st[y].score >= k + 64u) --y;
    }
}

// The result once the columns are done: d from the last column when every word is active, else > k.
template <typename Word>
STRSIM_HD uint64_t dist_final(const Word *st, int y, uint32_t W, uint64_t m, uint64_t nt, uint64_t k)
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

// One pair per lane.  TR: 1 = OSA, 0 = Levenshtein.  LIT: 0 = row against row, 1 = a is a literal (rowsA == 1), 2 = b is
// (lane_pick of strsim_wave_util.h: a literal is the text).  OUT: uint32_t = the distance under the cutoff kcut, a row whose
// lengths differ by more than it is kcut + 1 without the DP, and a wave of such rows runs no columns; double = the similarity
// (kcut is not looked at).  Rows this kernel cannot take are appended to `worklist`; st->wave_rows counts them and st->max_len
// bounds their patterns (min of the two byte lengths).  The status block is zeroed before the launch.
template <bool TR, int LIT, typename OUT>
__global__ __launch_bounds__(256) void k_dist_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA,
                                                   const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t n,
                                                   uint32_t kcut, OUT *__restrict__ out, uint32_t *__restrict__ worklist, DevStatus *st)
{
    constexpr bool SIM = std::is_same<OUT, double>::value;
    const uint32_t k = SIM ? DIST_UNBOUNDED : kcut;
    const LaneRow r = lane_row(offA, offB, n, LIT == 1, LIT == 2);
    const uint64_t row = r.row;
    const uint32_t la = r.la, lb = r.lb;
    const bool fits = r.live && dist_lane_fits(la, lb);
    const LanePick p = lane_pick<LIT>(valA, valB, r);
    const uint32_t lp = p.lp, lt = p.lt;
    uint32_t wp[16] = {}, wt[16] = {};
    bool ascii = false;
    if (fits) {
        osa_load64(p.pv, p.po, lp, wp);
        osa_load64(p.tv, p.to, lt, wt);
        ascii = (osa_high_bits(wp) | osa_high_bits(wt)) == 0u;
    }
    const uint32_t cls = dist_lane_row(r.live, la, lb, ascii, k);
    worklist_append<false>(cls == DIST_ROW_WAVE, row, la, lb, worklist, st); // rows for k_dist_wave
    if constexpr (!SIM)
        if (cls == DIST_ROW_CUT) out[row] = k + 1u;
    const bool run = cls == DIST_ROW_RUN;
    if (__ballot(run) == 0ull) return;
    const uint32_t tmax = osa_wave_max(run ? lt : 0u);
    const uint32_t pmax = osa_wave_max(run ? lp : 0u);
    uint32_t Plo[7], Phi[7];
    osa_planes(wp, Plo, Phi, pmax > 32u);
    // (a row the cutoff decided has its text loaded and runs no column; without a cutoff there is none, and a literal's length stays
    // a uniform value)
    const uint32_t cols = (SIM || run) ? lt : 0u;
    uint32_t d;
    if (pmax <= 32u) d = dist_lane_core<uint32_t, TR>(wt, cols, tmax, Plo, Phi, lp);
    else d = dist_lane_core<uint64_t, TR>(wt, cols, tmax, Plo, Phi, lp);
    if (run) out[row] = dist_result<OUT>(d, la, lb, k);
}

// One pair per wave (blockDim.x = 64) for the rows k_dist_lane put on the work list (st->wave_rows of them).  scratch: gridDim.x
// slots of slot_words words for patterns of more than OSA_WAVE_LDS_CPS values (nullptr when the call has none).  OUT as k_dist_lane.
template <bool TR, typename OUT>
__global__ __launch_bounds__(64) void k_dist_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                  const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB,
                                                  uint32_t kcut, OUT *__restrict__ out, const uint32_t *__restrict__ worklist,
                                                  const DevStatus *st, uint32_t *scratch, uint64_t slot_words)
{
    constexpr bool SIM = std::is_same<OUT, double>::value;
    const uint32_t k = SIM ? DIST_UNBOUNDED : kcut;
    __shared__ uint32_t s_pat[OSA_WAVE_LDS_CPS];
    using Word = std::conditional_t<SIM, DistWordFree, DistWord>;
    __shared__ Word s_state[OSA_WAVE_LDS_CPS / 64u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = st->wave_rows;
    for (uint32_t r = blockIdx.x; r < count; r += gridDim.x) {
        const WavePair p = wave_pair(offA, valA, rowsA, offB, valB, rowsB, worklist[r]);
        const WaveStage<Word> s = wave_stage(p, s_pat, s_state, OSA_WAVE_LDS_CPS, scratch, slot_words);
        const uint32_t m = s.m, nt = s.nt, W = s.W;
        uint64_t d = nt;
        if (!SIM && dist_length_cut(m, nt, k)) {
            d = (uint64_t)k + 1u;
        } else if (m != 0u) {
            const bool bounded = !SIM && k < nt; // (d <= nt: a larger k cuts nothing)
            wave_pattern(s.pp, s.pbytes, m, W, s.pat, lane);
            int y = dist_first_y(W, m, k, bounded);
            for (uint32_t w = lane; w < W; w += 64u) s.state[w] = dist_word_start<Word>(w);
            __syncthreads();
            uint64_t c = 0u;
            const bool done = wave_each_char(s.tp, s.tbytes, lane, [&](uint32_t ch) {
                dist_column<TR>(s.state, y, W, k, c, bounded, [&](uint32_t w) { return (uint64_t)__ballot(s.pat[64u * w + lane] == ch); });
                ++c;
                return SIM || !(y < 0 && c > k); // false: no cell of this column is <= k (row 0 holds c), the pair is decided
            });
            d = done ? dist_final(s.state, y, W, m, nt, k) : (uint64_t)k + 1u;
            __syncthreads(); // (the next row overwrites pat / state)
        }
        if (lane == 0u) out[p.row] = dist_result<OUT>(d, p.ca, p.cb, k);
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
