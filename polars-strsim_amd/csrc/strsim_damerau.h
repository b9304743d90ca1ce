// strsim_damerau.h -- unrestricted Damerau-Levenshtein similarity and distance (strsim_damerau_device / _host,
// strsim_damerau_distance_device / _host).  It has no measure id.
//
// d(a, b) is the smallest number of insertions, deletions, substitutions and swaps of two adjacent characters that turns a into b
// over Unicode scalar values; a substring may be edited any number of times (Lowrance and Wagner 1975), so ("ca", "abc") is 2 where
// the restricted measure of strsim_osa.h gives 3, and d is a metric.  The similarity is epilogue_osa of d; with a cutoff k the
// distance is d when d <= k and k + 1 otherwise (dist_result of strsim_distance.h).
//
// There is no bit-parallel form.  The kernels run the linear-space cell DP of Zhao and Sahni, with the table indexed by character
// replaced by state that travels with the column.  Rows are a_1..a_m, columns b_1..b_n; per column j the walk keeps
//   P1 = D[i-1][j], P2 = D[i-2][j], K = the last row k < i with a_k == b_j (0: none), FR = D[k-1][j-2] of that row k,
// and per row i
//   l = the last column < j with a_i == b_l (0: none), T = D[i-2][l-1] of that column l,
// so that a cell is
//   v = min(D[i-1][j-1] + (a_i != b_j), D[i][j-1] + 1, D[i-1][j] + 1)
//   on a mismatch with l, k >= 1:  l == j - 1 -> v = min(v, FR + (i - k));  else k == i - 1 -> v = min(v, T + (j - l))
// (dl_cell).  K[j] is the character table's entry for b_j, read at the only place the table is ever read: in column j.  The two
// transposition terms are guarded by l, k >= 1 and not by a large start value, so nothing is ever added to a sentinel and every
// stored value is a true cell of D, at most max(m, n).
//
// Two tiers, both finished in stream order:
//   k_dl_lane<LIT, OUT>  one pair per lane, both strings ASCII and <= DL_LANE_MAX bytes.  The column state of a lane is one packed
//                        dword a column in LDS, laid out [column][lane]; the outer loop runs over the pattern of lane_pick (the
//                        longer string, or the row string beside a literal), the inner one over the text.  Every other row is
//                        appended to the work list.
//   k_dl_wave<CAP, OUT>  one pair per wave for the work list: any UTF-8, any length.  Systolic: the longer string is cut into strips
//                        of 64 rows, one a lane; the shorter one streams through the lanes, lane r working on column t - r at step
//                        t, and the column state moves from lane r - 1 to lane r by a cross-lane shift.  Lane 63's outgoing state is
//                        the boundary row of the next strip: in LDS up to CAP columns, in the context's scratch beyond.
#pragma once
#include <stdint.h>
#include <type_traits>

#include "strsim_bounds.h"
#include "strsim_distance.h"

namespace strsim {

constexpr uint32_t DL_LANE_MAX = 32u;        // k_dl_lane: both strings ASCII and at most this long
constexpr uint32_t DL_WAVE_SMALL_COLS = 256u; // k_dl_wave<CAP>: the two sizes of the boundary row held in LDS, in columns
constexpr uint32_t DL_WAVE_LDS_COLS = 2048u;
constexpr uint32_t DL_COL_WORDS = 5u;        // words of a column in the boundary row: the character, P1, P2, FR, K

// what travels with column j
struct DlCol {
    uint32_t p1, p2, fr, k, ch;
};
// what stays with row i: its character, D[i][j-1], D[i-1][j-1], D[i-1][j-2], D[i-2][j-1], l and T
struct DlRow {
    uint32_t ch, i, left, d1, d2, q2, l, T;
};

STRSIM_HD uint32_t dl_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// column j before the first row (D[0][j] = j), row i before the first column (D[i][0] = i, D[i-1][0] = i - 1, D[i-2][0] = i - 2)
STRSIM_HD DlCol dl_col_start(uint32_t j, uint32_t ch) { return DlCol{j, 0u, 0u, 0u, ch}; }
STRSIM_HD DlRow dl_row_start(uint32_t i, uint32_t ch) { return DlRow{ch, i, i, i - 1u, 0u, i >= 2u ? i - 2u : 0u, 0u, 0u}; }

// cell (r.i, j): c comes in as the column's state above the cell and leaves as its state below it
STRSIM_HD void dl_cell(DlRow &r, DlCol &c, uint32_t j)
{
    const bool match = r.ch == c.ch;
    const uint32_t up = c.p1;
    uint32_t v = dl_min(dl_min(r.d1 + (match ? 0u : 1u), r.left + 1u), up + 1u);
    if (match) {
        c.fr = r.d2;
        r.T = r.q2;
        r.l = j;
        c.k = r.i;
    } else if (r.l >= 1u && c.k >= 1u) {
        if (r.l == j - 1u) v = dl_min(v, c.fr + (r.i - c.k));
        else if (c.k == r.i - 1u) v = dl_min(v, r.T + (j - r.l));
    }
    r.d2 = r.d1;
    r.d1 = up;
    r.q2 = c.p2;
    c.p2 = up;
    c.p1 = v;
    r.left = v;
}

// ---- the lane core ----

// A lane's column in one dword: P1, P2, FR and K are cells of D or row numbers, at most DL_LANE_MAX (6 bits each), the character
// is ASCII (7 bits).
static_assert(DL_LANE_MAX < 64u, "a packed field holds 6 bits");
STRSIM_HD uint32_t dl_pack(const DlCol &c) { return c.p1 | (c.p2 << 6) | (c.fr << 12) | (c.k << 18) | (c.ch << 24); }
STRSIM_HD DlCol dl_unpack(uint32_t w) { return DlCol{w & 63u, (w >> 6) & 63u, (w >> 12) & 63u, (w >> 18) & 63u, w >> 24}; }

// The window w moved down by one byte: w[0] & 0xFF is then the next character.  (A walk over the bytes by shifting, not by an index:
// an index into the registers that is not a constant would put the window into private memory.)
STRSIM_HD void dl_next_byte(uint32_t (&w)[8])
{
#pragma unroll
    for (int d = 0; d < 7; ++d) w[d] = (w[d] >> 8) | (w[d + 1] << 24);
    w[7] >>= 8;
}

// d of the rows wp (lp bytes) against the columns wt (lt bytes), both ASCII and <= DL_LANE_MAX.  col[(j - 1) * stride] is the
// lane's record of column j.  pmax / tmax: the loop bounds (the same in every lane, >= lp / lt); the cells beyond a lane's own
// strings are predicated off.
STRSIM_HD uint32_t dl_lane_core(const uint32_t (&wp)[8], uint32_t lp, uint32_t pmax, const uint32_t (&wt)[8], uint32_t lt, uint32_t tmax,
                                uint32_t *col, uint32_t stride)
{
    uint32_t w[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) w[d] = wt[d];
    for (uint32_t j = 1u; j <= tmax; ++j) {
        col[(j - 1u) * stride] = dl_pack(dl_col_start(j, w[0] & 0xFFu));
        dl_next_byte(w);
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) w[d] = wp[d];
    uint32_t d = lp + lt; // (one of them is empty)
    for (uint32_t i = 1u; i <= pmax; ++i) {
        DlRow row = dl_row_start(i, w[0] & 0xFFu);
        dl_next_byte(w);
        for (uint32_t j = 1u; j <= tmax; ++j) {
            if (i <= lp && j <= lt) {
                DlCol c = dl_unpack(col[(j - 1u) * stride]);
                dl_cell(row, c, j);
                col[(j - 1u) * stride] = dl_pack(c);
            }
        }
        if (i == lp && lt != 0u) d = row.left;
    }
    return d;
}

// What k_dl_lane does with a row (DistRow of strsim_distance.h); ascii is only looked at for a row that fits.
STRSIM_HD bool dl_lane_fits(uint32_t la, uint32_t lb) { return la <= DL_LANE_MAX && lb <= DL_LANE_MAX; }
STRSIM_HD uint32_t dl_lane_row(bool live, uint32_t la, uint32_t lb, bool ascii, uint32_t k)
{
    if (!live) return DIST_ROW_NONE;
    if (!dl_lane_fits(la, lb) || !ascii) return DIST_ROW_WAVE;
    return dist_length_cut(la, lb, k) ? DIST_ROW_CUT : DIST_ROW_RUN;
}

// ---- the strip walk ----
//
// The m rows are cut into strips of 64; strip s holds rows 64 s + 1 .. 64 s + rs, one a lane.  The n columns pass through it in
// n + rs - 1 steps: at step t (from 0) lane r has column t - r + 1.  The boundary row under a strip is kept per column, in place:
// the walk reads columns 64 c + 1 .. 64 c + 64 of it at step 64 c (before lane 0 needs the first of them) and has the last of
// them back from lane 63 at step 64 c + 126.

STRSIM_HD uint32_t dl_strips(uint64_t m) { return (uint32_t)((m + 63u) / 64u); }
STRSIM_HD uint32_t dl_strip_rows(uint64_t m, uint32_t s) { return (uint32_t)(m - 64u * (uint64_t)s >= 64u ? 64u : m - 64u * (uint64_t)s); }
STRSIM_HD uint32_t dl_strip_steps(uint32_t n, uint32_t rs) { return n + rs - 1u; }

// the column of lane r at step t (1-based), 0 when it has none
STRSIM_HD uint32_t dl_strip_col(uint32_t r, uint32_t t, uint32_t rs, uint32_t n)
{
    return (r < rs && t >= r && t - r < n) ? t - r + 1u : 0u;
}

// One step of one lane: `c` is what the lane above handed down (lane 0: the boundary row's column) and leaves as what this lane
// hands down.  -> the column, 0 when the lane had none (c then passes through unchanged).
STRSIM_HD uint32_t dl_strip_step(DlRow &row, DlCol &c, uint32_t r, uint32_t t, uint32_t rs, uint32_t n)
{
    const uint32_t j = dl_strip_col(r, t, rs, n);
    if (j != 0u) dl_cell(row, c, j);
    return j;
}

// Words of scratch of one k_dl_wave wave for pairs whose shorter string has up to n scalar values.
STRSIM_HD uint64_t dl_wave_slot_words(uint64_t n) { return (uint64_t)DL_COL_WORDS * n; }

#if defined(__HIPCC__) && !defined(STRSIM_OSA_NO_KERNELS)
// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------

// One pair per lane.  LIT and OUT as k_dist_lane: a literal is the text (the columns), read through a wave-uniform address;
// OUT = uint32_t is the distance under the cutoff kcut, a row whose lengths differ by more than it is kcut + 1 without the DP and a
// wave of such rows runs no cells; OUT = double is the similarity (kcut is not looked at).  Rows this kernel cannot take are
// appended to `worklist`; st->wave_rows counts them and st->max_len bounds their shorter strings (bytes).  The status block is
// zeroed before the launch.
template <int LIT, typename OUT>
__global__ __launch_bounds__(256) void k_dl_lane(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA,
                                                 const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t n, uint32_t kcut,
                                                 OUT *__restrict__ out, uint32_t *__restrict__ worklist, DevStatus *st)
{
    constexpr bool SIM = std::is_same<OUT, double>::value;
    __shared__ uint32_t s_col[DL_LANE_MAX * 256u]; // [column][lane]: a wave reads and writes 64 consecutive dwords
    const uint32_t k = SIM ? DIST_UNBOUNDED : kcut;
    const LaneRow r = lane_row(offA, offB, n, LIT == 1, LIT == 2);
    const uint32_t la = r.la, lb = r.lb;
    const bool fits = r.live && dl_lane_fits(la, lb);
    const LanePick p = lane_pick<LIT>(valA, valB, r);
    uint32_t wp[8] = {}, wt[8] = {};
    bool ascii = false;
    if (fits) {
        load_window32(p.pv, p.po, p.po + p.lp, wp);
        load_window32(p.tv, p.to, p.to + p.lt, wt);
        uint32_t o = 0u;
#pragma unroll
        for (int d = 0; d < 8; ++d) o |= wp[d] | wt[d];
        ascii = (o & 0x80808080u) == 0u;
    }
    const uint32_t cls = dl_lane_row(r.live, la, lb, ascii, k);
    worklist_append<false>(cls == DIST_ROW_WAVE, r.row, la, lb, worklist, st); // rows for k_dl_wave
    if constexpr (!SIM)
        if (cls == DIST_ROW_CUT) out[r.row] = k + 1u;
    const bool run = cls == DIST_ROW_RUN;
    if (__ballot(run) == 0ull) return;
    const uint32_t lp = run ? p.lp : 0u, lt = run ? p.lt : 0u;
    const uint32_t pmax = osa_wave_max(lp), tmax = osa_wave_max(lt);
    STRSIM_CHECK_RANGE(K_DAMERAU, 1, r.row, pmax, 0, DL_LANE_MAX);
    STRSIM_CHECK_RANGE(K_DAMERAU, 2, r.row, tmax, 0, DL_LANE_MAX);
    STRSIM_CHECK_INDEX(K_DAMERAU, 3, r.row, (tmax ? tmax - 1u : 0u) * 256u + threadIdx.x, DL_LANE_MAX * 256u);
    const uint32_t d = dl_lane_core(wp, lp, pmax, wt, lt, tmax, s_col + threadIdx.x, 256u);
    if (run) out[r.row] = dist_result<OUT>(d, la, lb, k);
}

__device__ __forceinline__ DlCol dl_shift_down(const DlCol &c)
{
    return DlCol{(uint32_t)__shfl_up((int)c.p1, 1, 64), (uint32_t)__shfl_up((int)c.p2, 1, 64), (uint32_t)__shfl_up((int)c.fr, 1, 64),
                 (uint32_t)__shfl_up((int)c.k, 1, 64), (uint32_t)__shfl_up((int)c.ch, 1, 64)};
}

// Strip s (rs rows, this lane's character mych) over the n columns whose characters are vals[0 .. n).  bnd: the boundary row, four
// arrays of `pitch` words (P1, P2, FR, K) behind one another, read when s > 0 and written when `more` strips follow.  s_in / s_out
// stage 64 columns of it.  -> D[64 s + r + 1][n] in lane r < rs.
__device__ __forceinline__ uint32_t dl_wave_strip(uint32_t s, uint32_t rs, uint32_t mych, bool more, uint32_t n, const uint32_t *vals,
                                                  uint32_t *bnd, uint64_t pitch, uint32_t *s_in, uint32_t *s_out, uint32_t lane, uint32_t row)
{
    DlRow rw = dl_row_start(64u * s + lane + 1u, mych);
    DlCol c = dl_col_start(0u, 0u);
    const uint32_t steps = dl_strip_steps(n, rs);
    for (uint32_t t = 0u; t < steps; ++t) {
        if ((t & 63u) == 0u) {
            // columns t + 1 .. t + 64 of the boundary row into the stage
            const uint32_t idx = t + lane;
            DlCol b = dl_col_start(idx + 1u, 0u);
            if (idx < n) {
                STRSIM_CHECK_INDEX(K_DAMERAU, 10, row, idx, pitch);
                b.ch = vals[idx];
                if (s != 0u) {
                    b.p1 = bnd[idx];
                    b.p2 = bnd[pitch + idx];
                    b.fr = bnd[2u * pitch + idx];
                    b.k = bnd[3u * pitch + idx];
                }
            }
            __syncthreads(); // (lane 0 has read the stage's last column)
            s_in[lane] = b.p1;
            s_in[64u + lane] = b.p2;
            s_in[128u + lane] = b.fr;
            s_in[192u + lane] = b.k;
            s_in[256u + lane] = b.ch;
            __syncthreads();
        }
        c = dl_shift_down(c);
        if (lane == 0u) {
            const uint32_t x = t & 63u;
            c = DlCol{s_in[x], s_in[64u + x], s_in[128u + x], s_in[192u + x], s_in[256u + x]};
        }
        const uint32_t j = dl_strip_step(rw, c, lane, t, rs, n);
        if (more) {
            // lane 63 fills the outgoing stage; a full one, or the row's last, goes to the boundary row
            const uint32_t j63 = dl_strip_col(63u, t, rs, n); // (the same in every lane)
            if (j63 != 0u) {
                const uint32_t x = (j63 - 1u) & 63u;
                if (lane == 63u) {
                    STRSIM_CHECK_RANGE(K_DAMERAU, 11, row, j, j63, j63);
                    s_out[x] = c.p1;
                    s_out[64u + x] = c.p2;
                    s_out[128u + x] = c.fr;
                    s_out[192u + x] = c.k;
                }
                if (x == 63u || j63 == n) {
                    __syncthreads();
                    const uint32_t idx = (j63 - 1u) - x + lane;
                    if (lane <= x) {
                        STRSIM_CHECK_INDEX(K_DAMERAU, 12, row, idx, n);
                        bnd[idx] = s_out[lane];
                        bnd[pitch + idx] = s_out[64u + lane];
                        bnd[2u * pitch + idx] = s_out[128u + lane];
                        bnd[3u * pitch + idx] = s_out[192u + lane];
                    }
                    __syncthreads();
                }
            }
        }
        (void)j;
    }
    __syncthreads(); // (the next strip reads what this one stored)
    return rw.left;
}

// One pair per wave (blockDim.x = 64) for the rows k_dl_lane put on the work list (st->wave_rows of them).  The string with fewer
// scalar values gives the columns, held with the boundary row in LDS up to CAP values; scratch: gridDim.x slots of slot_words words
// for longer ones (nullptr when the call has none).  OUT as k_dl_lane.
template <uint32_t CAP, typename OUT>
__global__ __launch_bounds__(64) void k_dl_wave(const uint32_t *__restrict__ offA, const uint8_t *__restrict__ valA, uint64_t rowsA,
                                                const uint32_t *__restrict__ offB, const uint8_t *__restrict__ valB, uint64_t rowsB, uint32_t kcut,
                                                OUT *__restrict__ out, const uint32_t *__restrict__ worklist, const DevStatus *st,
                                                uint32_t *scratch, uint64_t slot_words)
{
    constexpr bool SIM = std::is_same<OUT, double>::value;
    const uint32_t k = SIM ? DIST_UNBOUNDED : kcut;
    __shared__ uint32_t s_row[DL_COL_WORDS * CAP];
    __shared__ uint32_t s_in[DL_COL_WORDS * 64u], s_out[4u * 64u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = st->wave_rows;
    for (uint32_t r = blockIdx.x; r < count; r += gridDim.x) {
        STRSIM_CHECK_INDEX(K_DAMERAU, 20, r, worklist[r], rowsA > rowsB ? rowsA : rowsB);
        const WavePair p = wave_pair(offA, valA, rowsA, offB, valB, rowsB, worklist[r]);
        // the rows are the string with more scalar values (m of them), the columns the other (n)
        const bool a_rows = p.ca >= p.cb;
        const uint8_t *rp = a_rows ? p.pa : p.pb, *cp = a_rows ? p.pb : p.pa;
        const uint32_t rbytes = a_rows ? p.na : p.nb, cbytes = a_rows ? p.nb : p.na;
        const uint32_t m = a_rows ? p.ca : p.cb, n = a_rows ? p.cb : p.ca;
        uint64_t d = m; // (n == 0)
        if (!SIM && dist_length_cut(m, n, k)) {
            d = (uint64_t)k + 1u;
        } else if (n != 0u) {
            uint32_t *vals = s_row;
            uint64_t pitch = CAP;
            if (n > CAP) {
                STRSIM_CHECK_RANGE(K_DAMERAU, 21, p.row, (uint64_t)DL_COL_WORDS * n, 0, slot_words);
                vals = scratch + (uint64_t)blockIdx.x * slot_words;
                pitch = slot_words / DL_COL_WORDS;
            }
            uint32_t *bnd = vals + pitch;
            wave_decode(cp, cbytes, vals, lane);
            __syncthreads();
            const uint32_t strips = dl_strips(m);
            uint32_t cnt = 0u, mych = 0u, last = 0u;
            wave_each_char(rp, rbytes, lane, [&](uint32_t ch) {
                if (lane == (cnt & 63u)) mych = ch;
                ++cnt;
                if ((cnt & 63u) == 0u || cnt == m) {
                    const uint32_t s = (cnt - 1u) / 64u;
                    last = dl_wave_strip(s, dl_strip_rows(m, s), mych, s + 1u < strips, n, vals, bnd, pitch, s_in, s_out, lane, p.row);
                }
            });
            d = (uint32_t)__shfl((int)last, (int)((m - 1u) & 63u), 64);
        }
        if (lane == 0u) out[p.row] = dist_result<OUT>(d, p.ca, p.cb, k);
    }
}
#endif // __HIPCC__ && !STRSIM_OSA_NO_KERNELS

} // namespace strsim
