// strsim_kernels.hip -- gfx950 (MI355X / CDNA4) kernels for the five pairwise string-similarity
// measures of polars-strsim (reference src/expressions/strsim.rs:109-345).
//
// Device data layout (per column shard): uint32 offsets[rows+1] + packed UTF-8 bytes; output f64[n].
//
// Kernels, chained through one 64-bit "not finished yet" mask per 64 rows:
//
//   k_lane_stage<M>   ONE PAIR PER LANE, strings <= 32 ASCII bytes (the dominant kernel; strsim_lane_stage.h).  A persistent
//                     256-thread workgroup copies the contiguous byte range of a block of up to 512 rows into LDS with
//                     LDS-DMA, buckets the rows by DP column count and runs them as rounds of 64 rows of similar length:
//                     each lane picks its two 32-byte windows out of LDS, transposes one into bit-planes and runs the
//                     bit-parallel cores of strsim_lane_core.h in registers.  k_lane_stage_all: five outputs from one pass.
//   k_lane_lit<M>     a column against a Utf8 literal (strsim_lane_lit.h): the literal is the wave-uniform text.
//   k_lane_wide<M>    ONE PAIR PER LANE, 33..128 ASCII bytes: the same cores with masks of 1..4 words -- as wide as the PATTERN
//                     (strsim_lane_wide.h); the rows of a 16 384-row super sorted by (mask words, columns to run), a round's
//                     windows fetched by the wave together through its LDS rows, where the text stays.
//   k_lane_utf8<M>    ONE PAIR PER LANE, short non-ASCII strings (<= 32 scalar values, BMP): per-lane UTF-8 decode
//                     into 16-bit symbols in LDS, then the same cores on symbols (strsim_lane_sym.h).
//   k_wave_pairs<M>   the rest, up to WAVE_CAP bytes, any UTF-8, taken chunk by chunk from a work list k_lane_utf8 builds
//                     (strsim_kernel_wave.h; what only Levenshtein uses: strsim_wave_lev.h).
//                     Levenshtein: up to 16 pairs per wave in runs of lanes, block-parallel Myers (one 64-row block per
//                     lane, DPP hand-off), match masks from a per-lane LDS table, texts in a global arena; on bytes
//                     (ASCII) or on 16-bit scalar values (the reference works on `char`s, strsim.rs:133,189,297).
//                     Other measures: one pair per wave, scalar values in LDS, ballot matching / histograms.
//   k_dist_lane / k_dist_wave  the edit distances over scalar values (strsim_distance.h): one pair per lane for ASCII strings of up
//                     to 64 bytes, one pair per wave for the rest; both in stream order, no second pass.  As uint32: the bounded
//                     Levenshtein and OSA distances, with a length prefilter and, in the wave tier, the block cutoff of Myers /
//                     Ukkonen.  As double: the optimal string alignment similarity (measure 6, strsim_osa.h), never a cutoff.
//   k_indel_lane / k_indel_wave  Indel (LCS) similarity and distance (measure 8, strsim_indel.h): one pair per lane for ASCII
//                     strings of up to 128 bytes (1..4 mask words per wave), one pair per wave for the rest; in stream order.
//   k_qgram_lane / k_qgram_wave  q-gram Jaccard, Dice, overlap and cosine (strsim_qgram.h; q = 1..3, multiset or set): one pair per
//                     lane for ASCII strings of up to 64 bytes (gram masks from shifted match masks), one pair per wave through a
//                     hash table of the grams of both strings for the rest; in stream order.
//   k_dl_lane / k_dl_wave  unrestricted Damerau-Levenshtein similarity and distance (strsim_damerau.h): a cell DP, not a bit-parallel
//                     step.  One pair per lane for ASCII strings of up to 32 bytes, the column state packed into one dword a
//                     column in LDS; one pair per wave for the rest, systolic over strips of 64 rows; in stream order.
//   k_common_lane / k_common_wave  Hamming, prefix and postfix similarity, distance and count (strsim_common.h): one pair per lane
//                     for ASCII strings of up to 32 bytes, a mask of the differing bytes of the two windows; one pair per wave for
//                     the rest, streamed 64 bytes at a time.  k_common_lcs_lane / k_common_lcs_wave: LCSseq on strsim_indel.h's
//                     bit-parallel step.  In stream order.
//   k_partial_lane / k_partial_wave  partial ratio and its alignment (measure 10, strsim_partial.h): the best window of the longer
//                     string against the shorter one, match masks built once per pair; ASCII strings of up to 32 bytes per lane,
//                     the rest one pair per wave; in stream order.
//   k_token_sort_* / k_token_set_*  token_sort_ratio and token_set_ratio (measures 14 and 16, strsim_token.h): tokenise, sort and
//                     join (or merge as sets) every string into scratch columns that k_indel_lane / k_indel_wave then align;
//                     ASCII strings of up to 64 bytes and 16 tokens per lane, the rest one string per wave.
//   k_process_lane / k_process_wave  default_process (strsim_process.h): the column transform in front of processed scoring, a
//                                   measuring and a writing pass around the token transforms' offset scan
//   k_wratio_classify / k_take_* / k_wratio_combine  WRatio (measure 26, strsim_wratio.h): a row's class from the lengths of its
//                     raw strings, the near and the far rows gathered into sub-frames for the token and the partial family, the
//                     rule per row; k_max_f64 and k_partial_token_set_epilogue close token_ratio and the partial token ratios
//                     (measures 18 .. 24), which are compositions of the kernels above.
//   k_nearest_lane<TR, K> / k_extract_lane<K>  the two length-ordered searches, one sweep (search_sweep_lane,
//                     strsim_nearest_kernels.h) under two rule sets: one query per lane in length order against wave-uniform
//                     candidates, a candidate length window and a running bound per lane.  Nearest match by bounded edit
//                     distance (NearestRules, strsim_nearest.h); top-k by Indel similarity with a score cutoff, scores ordered
//                     through a rank table in LDS (ExtractRules, strsim_extract.h; strsim_extract_kernels.h).
//   k_cdist_lane<M>   the full score matrix (strsim_cdist.h, strsim_cdist_kernels.h): k_match_lane's sweep with every score kept,
//                     staged per wave in a tile of LDS and written out row-wise; k_cdist_put_col / k_cdist_cutoff close its fallback.
//   k_qgram_join_lane<Q, SET, FILL>  the threshold join by q-gram similarity (strsim_qgram_join.h, strsim_qgram_join_kernels.h): the
//                     join's lane sweep with the q-gram gram masks as its scoring call, the candidate as the wave-uniform text.
//   k_distance_join_lane<KIND, FILL>  the join by integer edit distance (strsim_distance_join.h, strsim_distance_join_kernels.h): the
//                     join's lane sweep with the Levenshtein / OSA column as its scoring call; Damerau-Levenshtein filters by the
//                     OSA distance and runs dl_lane_core for the wave when a lane is left undecided.
//   k_huge_pairs<M>   strings beyond WAVE_CAP, scratch in global memory, launched from strsim_ctx_synchronize() only
//                     when such rows were counted; Levenshtein: the block step in stripes of 64 blocks, any length.
//
// No MFMA anywhere: this is integer/byte work whose roofline is HBM bytes.
// Built with -ffp-contract=off so the f64 epilogues are bit-identical to the Rust source.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <cstdlib>
#include <stdint.h>
#include <type_traits>

#include "strsim_bounds.h"
#include "strsim_lane_core.h"
#include "strsim_lane_lut.h"
#include "strsim_lane_ptab.h"
#include "strsim_lane_wide.h"
#include "strsim_lane_sym.h"
#include "strsim_kernels.h"
#include "strsim_lane_common.h"
#include "strsim_osa.h"
#include "strsim_distance.h"
#include "strsim_indel.h"
#include "strsim_partial.h"
#include "strsim_qgram.h"
#include "strsim_damerau.h"
#include "strsim_common.h"
#include "strsim_token.h"
#include "strsim_wratio.h"
#include "strsim_process.h"
#include "strsim_nearest.h"
#include "strsim_extract.h"
#include "strsim_cdist.h"
#include "strsim_join.h"
#include "strsim_match_join.h"
#include "strsim_qgram_join.h"
#include "strsim_distance_join.h"
#include "strsim_components.h"

namespace strsim {

constexpr int ALL_MEASURES = 5; // MEASURE value of the fused five-output instantiation

struct OutPtrs {
    double *p[5]; // indexed by Measure; single-measure kernels use p[0]
};

#include "strsim_lane_stage.h"
#include "strsim_lane_lit.h"
#include "strsim_match.h"
#include "strsim_nearest_kernels.h"
#include "strsim_extract_kernels.h"
#include "strsim_cdist_kernels.h"
#include "strsim_join_kernels.h"
#include "strsim_match_join_kernels.h"
#include "strsim_qgram_join_kernels.h"
#include "strsim_distance_join_kernels.h"
#include "strsim_components_kernels.h"

#include "strsim_kernel_wide.h"
#include "strsim_kernel_utf8.h"
#include "strsim_kernel_wave.h"
#include "strsim_kernel_huge.h"

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// k_lane_wide / k_lane_utf8 geometry: spans (WIDE_SPAN / U8_SPAN mask words) per super-span and workgroups.  A super is what one
// workgroup tests for "anything to do" with a single barrier; full-size frames use the largest (8 spans), smaller
// ones shrink it until there are about two supers per RESIDENT workgroup (a.wide_grid = 3 per CU).  The launch
// itself may be much larger than what is resident (a.wide_grid_cap): workgroups that finish early are replaced by
// fresh ones instead of waiting for the longest grid-stride loop (cfg3: 12.4 -> 10.3 ms).
static void wide_geometry(const LaunchArgs &a, int span, uint32_t &sps, unsigned &grid)
{
    const uint64_t nchunks = (a.n + 63u) >> 6;
    const uint64_t nspans = (nchunks + (uint64_t)span - 1) / (uint64_t)span;
    const uint64_t want = 2u * (uint64_t)a.wide_grid;
    uint64_t k = nspans / (want ? want : 1u);
    if (k < 1u) k = 1u;
    if (k > (uint64_t)(WIDE_BLOCK / span)) k = WIDE_BLOCK / span;
    sps = (uint32_t)k;
    const uint64_t nsuper = (nspans + k - 1u) / k;
    grid = (unsigned)(nsuper < (uint64_t)a.wide_grid_cap ? nsuper : (uint64_t)a.wide_grid_cap);
}

// Persistent workgroups of k_lane_stage for a frame of nsb blocks: all that are resident when the frame is large; a frame
// of a few blocks per workgroup runs faster on FEWER workgroups -- the pipeline of a workgroup (offsets and bytes of the next
// block in flight behind the current one) only pays from its second block on, and every workgroup pays the prologue: a
// 1 M-row call takes 0.085 ms on 5 workgroups per CU and 0.051 ms on 2.  So: about four blocks per workgroup, but at least
// one workgroup per CU while there are blocks for them.
static uint64_t stage_launch_size(uint64_t nsb, uint64_t resident, uint64_t cus)
{
    constexpr uint64_t per = 4; // blocks per workgroup (round 3's sweep: 2 / 4 / 8 -> 0.051 / 0.046 / 0.049 ms per 1 M rows)
    uint64_t g = nsb / per;
    const uint64_t floor_ = nsb < cus ? nsb : cus;
    if (g < floor_) g = floor_;
    if (g > resident) g = resident;
    return g ? g : 1u;
}

template <int M>
static void launch_lane_t(const LaunchArgs &a)
{
    if (a.ev_lane0) (void)hipEventRecord(a.ev_lane0, a.stream);
    OutPtrs op{};
    op.p[0] = a.out;
    // a column against a literal (strsim_lane_lit.h): the literal is the wave-uniform text, the column is staged -- on either
    // side, for every measure ([r5] Jaro / Jaro-Winkler included: they are symmetric, strsim_lane_core.h)
    const bool lit_a = a.rowsA == 1 && a.rowsB != 1, lit_b = a.rowsB == 1 && a.rowsA != 1;
    const bool lit_path = lit_a || lit_b;
    if (lit_path && !a.no_literal_path) {
        const bool litA = lit_a;
        const uint64_t nlb = (a.n + (LIT_ROWS - 1)) / LIT_ROWS;
        const uint64_t want = (uint64_t)a.stage_grid * 3u; // ~15 workgroups per CU in the launch, 5 resident
        const uint64_t gl = nlb < want ? nlb : want;
        hipLaunchKernelGGL((k_lane_lit<M>), dim3((unsigned)gl), dim3(LIT_BLOCK), 0, a.stream, litA ? a.offB : a.offA,
                           litA ? a.valB : a.valA, litA ? a.offA : a.offB, litA ? a.valA : a.valB, a.out, a.n, a.slowmask,
                           a.status, a.qtab, a.sched);
        if (a.publish_host) hipLaunchKernelGGL(k_publish_lit, dim3(1), dim3(64), 0, a.stream, a.sched, a.publish_host, a.publish_ticket);
    } else {
        // bytes staged through LDS (strsim_lane_stage.h): persistent workgroups, one per resident slot
        const uint64_t nsb = (a.n + (STAGE_ROWS - 1)) / STAGE_ROWS;
        // (a.stage_grid counts STRSIM_STAGE_WAVES_PER_EU workgroups per CU; an instantiation that runs fewer gets its share)
        auto go = [&](auto tables, auto long_rows) {
            constexpr bool T = decltype(tables)::value, L = decltype(long_rows)::value;
            const uint64_t res = (uint64_t)a.stage_grid * (uint64_t)stage_waves_per_eu<M, T, L>() / (uint64_t)STRSIM_STAGE_WAVES_PER_EU;
            const uint64_t gs = stage_launch_size(nsb, res, (uint64_t)a.stage_grid / (uint64_t)STRSIM_STAGE_WAVES_PER_EU);
            // (neither side a literal: the instantiation that has no literal code in it, where the measure has one)
            constexpr bool C = stage_has_cols_only<M, T, L>();
            if (C && a.rowsA != 1 && a.rowsB != 1)
                hipLaunchKernelGGL((k_lane_stage<M, T, L, C>), dim3((unsigned)gs), dim3(STAGE_BLOCK), 0, a.stream, a.offA, a.valA, a.rowsA,
                                   a.offB, a.valB, a.rowsB, op, a.n, a.slowmask, a.status, a.qtab, a.sched, a.publish_host, a.publish_ticket);
            else
                hipLaunchKernelGGL((k_lane_stage<M, T, L>), dim3((unsigned)gs), dim3(STAGE_BLOCK), 0, a.stream, a.offA, a.valA, a.rowsA,
                                   a.offB, a.valB, a.rowsB, op, a.n, a.slowmask, a.status, a.qtab, a.sched, a.publish_host, a.publish_ticket);
        };
        if (a.long_rows) go(std::false_type{}, std::true_type{});
        else if constexpr (stage_uses_lut<M>()) go(std::true_type{}, std::false_type{});
        else go(std::false_type{}, std::false_type{});
    }
    if (a.ev_lane1) (void)hipEventRecord(a.ev_lane1, a.stream);
}

template <int M>
static void launch_slow_kernels(const LaunchArgs &a, double *out)
{
    const uint64_t nchunks = (a.n + 63u) >> 6;
    uint32_t sps, sps8;
    unsigned g3, g8;
    wide_geometry(a, WIDE_SPAN, sps, g3);
    wide_geometry(a, U8_SPAN, sps8, g8);
    // waves per CU: Levenshtein by its 8 KB table; Jaro by its 12.4 KB of LDS (12); Jaccard / Dice 16 (a.wave_grid)
    const uint64_t wg = M == LEVENSHTEIN ? (uint64_t)a.wave_grid_lev
                        : (M == JARO || M == JARO_WINKLER) ? (uint64_t)a.wave_grid * 3u / 4u : (uint64_t)a.wave_grid;
    const uint64_t g2 = nchunks < wg ? nchunks : wg;
    hipLaunchKernelGGL((k_lane_wide<M>), dim3(g3), dim3(WIDE_BLOCK), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB,
                       a.valB, a.rowsB, out, a.n, a.slowmask, sps);
    hipLaunchKernelGGL((k_lane_utf8<M>), dim3(g8), dim3(WIDE_BLOCK), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB,
                       a.valB, a.rowsB, out, a.n, a.slowmask, sps8, a.worklist, a.status);
    hipLaunchKernelGGL((k_wave_pairs<M>), dim3((unsigned)g2), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB,
                       a.valB, a.rowsB, out, a.n, a.slowmask, a.worklist, a.status, a.lev_ws);
}

// one measure: the slow-row kernels into the call's output column
template <int M>
static void launch_slow_t(const LaunchArgs &a)
{
    launch_slow_kernels<M>(a, a.out);
    if (a.ev_wave1) (void)hipEventRecord(a.ev_wave1, a.stream);
}


template <int M>
static void launch_pair(const LaunchArgs &a)
{
    launch_lane_t<M>(a);
    launch_slow_t<M>(a);
}

template <int M>
static void launch_huge_t(const LaunchArgs &a, uint32_t *ws, uint32_t cap, int grid)
{
    hipLaunchKernelGGL((k_huge_pairs<M>), dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB,
                       a.valB, a.rowsB, a.out, a.n, ws, cap);
}

hipError_t launch_huge(int measure, const LaunchArgs &a, uint32_t *ws, uint32_t cap, int grid)
{
    switch (measure) {
    case LEVENSHTEIN: launch_huge_t<LEVENSHTEIN>(a, ws, cap, grid); break;
    case JARO: launch_huge_t<JARO>(a, ws, cap, grid); break;
    case JARO_WINKLER: launch_huge_t<JARO_WINKLER>(a, ws, cap, grid); break;
    case JACCARD: launch_huge_t<JACCARD>(a, ws, cap, grid); break;
    case SORENSEN_DICE: launch_huge_t<SORENSEN_DICE>(a, ws, cap, grid); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// All five measures of one frame: one fused lane kernel (five outputs), then the slow-row kernels per measure,
// each starting from the same mask (k_lane_wide clears what it finishes, so the mask is restored in between).
hipError_t launch_lane_all_only(const LaunchArgs &a, double *const outs[5])
{
    if (a.n == 0) return hipSuccess;
    OutPtrs op{};
    for (int q = 0; q < 5; ++q) op.p[q] = outs[q];
    if (a.ev_lane0) (void)hipEventRecord(a.ev_lane0, a.stream);
    {
        // one staged pass, five outputs (strsim_lane_stage.h, MEASURE = ALL_MEASURES)
        const uint64_t nsb = (a.n + (STAGE_ROWS - 1)) / STAGE_ROWS;
        const uint64_t cap = (uint64_t)a.stage_grid * (uint64_t)stage_waves_per_eu<ALL_MEASURES, stage_uses_lut<ALL_MEASURES>()>() / (uint64_t)STRSIM_STAGE_WAVES_PER_EU; // resident workgroups
        const uint64_t gs = stage_launch_size(nsb, cap, (uint64_t)a.stage_grid / (uint64_t)STRSIM_STAGE_WAVES_PER_EU);
        hipLaunchKernelGGL(k_lane_stage_all, dim3((unsigned)gs), dim3(STAGE_BLOCK), 0, a.stream, a.offA, a.valA,
                           a.rowsA, a.offB, a.valB, a.rowsB, op, a.n, a.slowmask, a.status, a.qtab, a.sched, a.publish_host,
                           a.publish_ticket);
    }
    if (a.ev_lane1) (void)hipEventRecord(a.ev_lane1, a.stream);
    return hipGetLastError();
}

hipError_t launch_slow_all_only(const LaunchArgs &a, double *const outs[5], unsigned long long *mask_backup)
{
    if (a.n == 0) return hipSuccess;
    const uint64_t nchunks = (a.n + 63u) >> 6;
    hipError_t e = hipMemcpyAsync(mask_backup, a.slowmask, nchunks * sizeof(unsigned long long), hipMemcpyDeviceToDevice, a.stream);
    if (e != hipSuccess) return e;
    launch_slow_kernels<LEVENSHTEIN>(a, outs[LEVENSHTEIN]);
    for (int m = 1; m < 5; ++m) {
        e = hipMemcpyAsync(a.slowmask, mask_backup, nchunks * sizeof(unsigned long long), hipMemcpyDeviceToDevice, a.stream);
        if (e != hipSuccess) return e;
        switch (m) {
        case JARO: launch_slow_kernels<JARO>(a, outs[m]); break;
        case JARO_WINKLER: launch_slow_kernels<JARO_WINKLER>(a, outs[m]); break;
        case JACCARD: launch_slow_kernels<JACCARD>(a, outs[m]); break;
        default: launch_slow_kernels<SORENSEN_DICE>(a, outs[m]); break;
        }
    }
    if (a.ev_wave1) (void)hipEventRecord(a.ev_wave1, a.stream);
    return hipGetLastError();
}

hipError_t launch_pairs_all(const LaunchArgs &a, double *const outs[5], unsigned long long *mask_backup)
{
    hipError_t e = launch_lane_all_only(a, outs);
    if (e != hipSuccess) return e;
    return launch_slow_all_only(a, outs, mask_backup);
}

// waves of k_wave_pairs<levenshtein> a CU holds at once (its grid is persistent: a wave that is not resident would start on
// its static share of the work list only when another one leaves); 0 if the runtime cannot tell
int wave_lev_resident_per_cu()
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_wave_pairs<LEVENSHTEIN>, 64, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int lane_kernel_launches(int measure, const LaunchArgs &a)
{
    if (measure == 5) return 1;
    const bool lit_a = a.rowsA == 1 && a.rowsB != 1, lit_b = a.rowsB == 1 && a.rowsA != 1;
    const bool lit_path = lit_a || lit_b;
    return (lit_path && !a.no_literal_path) ? 2 : 1; // k_lane_lit + k_publish_lit
}

hipError_t launch_lane_only(int measure, const LaunchArgs &a)
{
    if (a.n == 0) return hipSuccess;
    switch (measure) {
    case LEVENSHTEIN: launch_lane_t<LEVENSHTEIN>(a); break;
    case JARO: launch_lane_t<JARO>(a); break;
    case JARO_WINKLER: launch_lane_t<JARO_WINKLER>(a); break;
    case JACCARD: launch_lane_t<JACCARD>(a); break;
    case SORENSEN_DICE: launch_lane_t<SORENSEN_DICE>(a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_slow_only(int measure, const LaunchArgs &a)
{
    if (a.n == 0) return hipSuccess;
    switch (measure) {
    case LEVENSHTEIN: launch_slow_t<LEVENSHTEIN>(a); break;
    case JARO: launch_slow_t<JARO>(a); break;
    case JARO_WINKLER: launch_slow_t<JARO_WINKLER>(a); break;
    case JACCARD: launch_slow_t<JACCARD>(a); break;
    case SORENSEN_DICE: launch_slow_t<SORENSEN_DICE>(a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_pairs(int measure, const LaunchArgs &a)
{
    if (a.n == 0) return hipSuccess;
    switch (measure) {
    case LEVENSHTEIN: launch_pair<LEVENSHTEIN>(a); break;
    case JARO: launch_pair<JARO>(a); break;
    case JARO_WINKLER: launch_pair<JARO_WINKLER>(a); break;
    case JACCARD: launch_pair<JACCARD>(a); break;
    case SORENSEN_DICE: launch_pair<SORENSEN_DICE>(a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The call's status block, copied to pinned host memory by a one-wave kernel: an SDMA/blit copy behind the last kernel costs
// a queue hand-over of 10-16 us per call, this costs ~2 us (visible to the host once the stream has been synchronised).
__global__ void k_publish_status(const DevStatus *__restrict__ src, DevStatus *__restrict__ dst, uint32_t ticket)
{
    const unsigned *s = reinterpret_cast<const unsigned *>(src);
    unsigned *d = reinterpret_cast<unsigned *>(dst);
    // (lane_left belongs to k_lane_stage's last workgroup, which writes the host copy itself; the ticket goes last)
    constexpr unsigned TICKET_WORD = offsetof(DevStatus, ticket) / 4, LEFT_WORD = offsetof(DevStatus, lane_left) / 4;
    if (threadIdx.x < sizeof(DevStatus) / 4 && threadIdx.x != TICKET_WORD && threadIdx.x != LEFT_WORD)
        __builtin_nontemporal_store(s[threadIdx.x], d + threadIdx.x);
    __threadfence_system();
    // the ticket goes last: a host that sees it sees the block (one wave: the stores above were issued before this one)
    if (threadIdx.x == 0u) __hip_atomic_store(&dst->ticket, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_publish_status(const DevStatus *src, DevStatus *dst_mapped, uint32_t ticket, hipStream_t stream)
{
    hipLaunchKernelGGL(k_publish_status, dim3(1), dim3(64), 0, stream, src, dst_mapped, ticket);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// best match (strsim_match.h)
// ------------------------------------------------------------------------------------------------
int match_lane_k(uint32_t k) { return k <= 1u ? 1 : (k <= 4u ? 4 : 16); }

static unsigned match_grid(uint64_t n) { return (unsigned)((n + MATCH_BLOCK - 1) / MATCH_BLOCK); }

hipError_t launch_match_pack(const uint32_t *off, const uint8_t *val, uint32_t rows, uint32_t *words, uint32_t *meta,
                             uint32_t *slow_list, uint32_t *slow_count, hipStream_t stream)
{
    if (rows == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_match_pack, dim3(match_grid(rows)), dim3(MATCH_BLOCK), 0, stream, off, val, rows, words, meta, slow_list, slow_count);
    return hipGetLastError();
}

// f(std::integral_constant<int, K>) at the K = 1, 4 or 16 a call with k slots runs at
template <class F>
static void with_lane_k(uint32_t k, F f)
{
    const int K = match_lane_k(k);
    if (K == 1) f(std::integral_constant<int, 1>{});
    else if (K == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 16>{});
}

// f(std::integral_constant<int, LIT>): which side of the call is a literal (0: neither, 1: A, 2: B)
template <class F>
static void with_literal(const LaunchArgs &a, F f)
{
    const int lit = a.rowsA == a.rowsB ? 0 : (a.rowsA == 1 ? 1 : 2);
    if (lit == 1) f(std::integral_constant<int, 1>{});
    else if (lit == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 0>{});
}
static dim3 lane_grid(const LaunchArgs &a) { return dim3((unsigned)((a.n + 255u) / 256u)); }

template <int M>
static void launch_match_lane_m(const MatchLaneArgs &a)
{
    with_lane_k(a.k, [&](auto K) {
        hipLaunchKernelGGL((k_match_lane<M, decltype(K)::value>), dim3(match_grid(a.nq), a.splits), dim3(MATCH_BLOCK), 0, a.stream, a.qwords,
                           a.qmeta, a.nq, a.cwords, a.cmeta, a.nc, a.per, a.qtab, a.min_score, a.pscore, a.pidx);
    });
}

hipError_t launch_match_lane(int measure, const MatchLaneArgs &a)
{
    switch (measure) {
    case LEVENSHTEIN: launch_match_lane_m<LEVENSHTEIN>(a); break;
    case JARO: launch_match_lane_m<JARO>(a); break;
    case JARO_WINKLER: launch_match_lane_m<JARO_WINKLER>(a); break;
    case JACCARD: launch_match_lane_m<JACCARD>(a); break;
    default: launch_match_lane_m<SORENSEN_DICE>(a); break;
    }
    return hipGetLastError();
}

hipError_t launch_match_clear(double *score, uint32_t *idx, uint64_t n, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_match_clear, dim3(match_grid(n)), dim3(MATCH_BLOCK), 0, stream, score, idx, n);
    return hipGetLastError();
}

hipError_t launch_match_fold_cols(uint32_t k, const double *scores, const uint32_t *qlist, uint32_t nb, uint32_t nc, double min_score,
                                  double *fscore, uint32_t *fidx, hipStream_t stream)
{
    if (nb == 0u) return hipSuccess;
    with_lane_k(k, [&](auto K) {
        hipLaunchKernelGGL(k_match_fold_cols<decltype(K)::value>, dim3(nb), dim3(MATCH_BLOCK), 0, stream, scores, qlist, nc, min_score, fscore, fidx);
    });
    return hipGetLastError();
}

hipError_t launch_match_fold_rows(uint32_t k, const double *scores, const uint32_t *clist, uint32_t nb, const uint32_t *qmeta, uint32_t nq,
                                  double min_score, double *fscore, uint32_t *fidx, hipStream_t stream)
{
    if (nb == 0u || nq == 0u) return hipSuccess;
    with_lane_k(k, [&](auto K) {
        hipLaunchKernelGGL(k_match_fold_rows<decltype(K)::value>, dim3(match_grid(nq)), dim3(MATCH_BLOCK), 0, stream, scores, clist, nb, qmeta, nq,
                           min_score, fscore, fidx);
    });
    return hipGetLastError();
}

hipError_t launch_match_merge(uint32_t k, const double *pscore, const uint32_t *pidx, uint32_t nl, uint32_t nq, uint32_t *out_index,
                              double *out_score, hipStream_t stream)
{
    if (nq == 0u) return hipSuccess;
    with_lane_k(k, [&](auto K) {
        hipLaunchKernelGGL(k_match_merge<decltype(K)::value>, dim3(match_grid(nq)), dim3(MATCH_BLOCK), 0, stream, pscore, pidx, nl, nq, k,
                           out_index, out_score);
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// nearest match (strsim_nearest_kernels.h)
// ------------------------------------------------------------------------------------------------
hipError_t launch_nearest_order(const NearestOrderArgs &a)
{
    if (a.nq) hipLaunchKernelGGL(k_nearest_hist, dim3(match_grid(a.nq)), dim3(MATCH_BLOCK), 0, a.stream, a.qmeta, a.nq, a.qhist);
    if (a.nc) hipLaunchKernelGGL(k_nearest_hist, dim3(match_grid(a.nc)), dim3(MATCH_BLOCK), 0, a.stream, a.cmeta, a.nc, a.chist);
    hipLaunchKernelGGL(k_nearest_scan, dim3(1), dim3(64), 0, a.stream, a.qhist, a.chist, a.qstart, a.cstart, a.qcur, a.ccur);
    if (a.nq)
        hipLaunchKernelGGL(k_nearest_scatter<0>, dim3(match_grid(a.nq)), dim3(MATCH_BLOCK), 0, a.stream, (const uint32_t *)nullptr, a.qmeta,
                           a.nq, a.qcur, a.qperm, (uint32_t *)nullptr, (uint32_t *)nullptr);
    if (a.nc)
        hipLaunchKernelGGL(k_nearest_scatter<1>, dim3(match_grid(a.nc)), dim3(MATCH_BLOCK), 0, a.stream, a.cwords, a.cmeta, a.nc, a.ccur,
                           a.sidx, a.swords, a.smeta);
    return hipGetLastError();
}

template <bool TR>
static void launch_nearest_lane_tr(const NearestLaneArgs &a)
{
    const SweepLaneArgs &s = a.s;
    with_lane_k(s.k, [&](auto K) {
        hipLaunchKernelGGL((k_nearest_lane<TR, decltype(K)::value>), dim3(match_grid(s.nq), s.splits), dim3(MATCH_BLOCK), 0, s.stream, s.qwords,
                           s.qmeta, s.qperm, s.qstart, s.nq, s.swords, s.smeta, s.sidx, s.cstart, a.max_distance, s.pscore, s.pidx);
    });
}

hipError_t launch_nearest_lane(int measure, const NearestLaneArgs &a)
{
    if (measure == OSA) launch_nearest_lane_tr<true>(a);
    else launch_nearest_lane_tr<false>(a);
    return hipGetLastError();
}

hipError_t launch_nearest_scores(const uint32_t *dist, uint64_t n, double *score, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_nearest_scores, dim3(match_grid(n)), dim3(MATCH_BLOCK), 0, stream, dist, n, score);
    return hipGetLastError();
}

hipError_t launch_nearest_finish(const double *score, const uint32_t *index, uint64_t n, uint32_t *dist, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_nearest_finish, dim3(match_grid(n)), dim3(MATCH_BLOCK), 0, stream, score, index, n, dist);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// extract (strsim_extract_kernels.h)
// ------------------------------------------------------------------------------------------------
hipError_t launch_extract_lane(const ExtractLaneArgs &a)
{
    const SweepLaneArgs &s = a.s;
    with_lane_k(s.k, [&](auto K) {
        hipLaunchKernelGGL(k_extract_lane<decltype(K)::value>, dim3(match_grid(s.nq), s.splits), dim3(MATCH_BLOCK), 0, s.stream, s.qwords, s.qmeta,
                           s.qperm, s.qstart, s.nq, s.swords, s.smeta, s.sidx, s.cstart, a.tab, a.rlimit, s.pscore, s.pidx);
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// cdist (strsim_cdist_kernels.h)
// ------------------------------------------------------------------------------------------------
template <int M>
static void launch_cdist_lane_m(const CdistLaneArgs &a)
{
    hipLaunchKernelGGL(k_cdist_lane<M>, dim3((unsigned)(((uint64_t)a.nq + CDIST_BLOCK - 1) / CDIST_BLOCK), a.splits), dim3(CDIST_BLOCK), 0, a.stream, a.qwords, a.qmeta, a.nq, a.cwords,
                       a.cmeta, a.nc, a.per, a.tab, a.cutoff, a.out, a.ld);
}

hipError_t launch_cdist_lane(int measure, const CdistLaneArgs &a)
{
    switch (measure) {
    case LEVENSHTEIN: launch_cdist_lane_m<LEVENSHTEIN>(a); break;
    case JARO: launch_cdist_lane_m<JARO>(a); break;
    case JARO_WINKLER: launch_cdist_lane_m<JARO_WINKLER>(a); break;
    case JACCARD: launch_cdist_lane_m<JACCARD>(a); break;
    case SORENSEN_DICE: launch_cdist_lane_m<SORENSEN_DICE>(a); break;
    default: launch_cdist_lane_m<INDEL>(a); break;
    }
    return hipGetLastError();
}

hipError_t launch_cdist_put_col(const double *scores, const uint32_t *clist, uint32_t nb, const uint32_t *qmeta, uint32_t nq, double cutoff,
                                double *out, uint64_t ld, hipStream_t stream)
{
    if (nb == 0u || nq == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_cdist_put_col, dim3(match_grid(nq), nb), dim3(MATCH_BLOCK), 0, stream, scores, clist, qmeta, nq, cutoff, out, ld);
    return hipGetLastError();
}

hipError_t launch_cdist_cutoff(double *out, const uint32_t *qlist, uint32_t nb, uint32_t nc, uint64_t ld, double cutoff, hipStream_t stream)
{
    if (nb == 0u || nc == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_cdist_cutoff, dim3(match_grid(nc), nb), dim3(MATCH_BLOCK), 0, stream, out, qlist, nc, ld, cutoff);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// threshold join (strsim_join_kernels.h)
// ------------------------------------------------------------------------------------------------
// f(std::bool_constant<FILL>): the count (false) or the fill (true) form of a join kernel
template <class F>
static void with_fill(bool fill, F f)
{
    if (fill) f(std::true_type{});
    else f(std::false_type{});
}

hipError_t launch_join_lane(bool fill, const JoinLaneArgs &a, const ExtractTable *tab, uint32_t rlimit)
{
    with_fill(fill, [&](auto FILL) {
        hipLaunchKernelGGL(k_join_lane<decltype(FILL)::value>, dim3(match_grid(a.nq), a.splits), dim3(MATCH_BLOCK), 0, a.stream, a.qwords, a.qmeta,
                           a.qperm, a.qstart, a.nq, a.swords, a.smeta, a.sidx, a.cstart, tab, rlimit, a.upper, a.cnt, a.map, a.map_words, a.map_shift,
                           a.indptr, a.out_index, a.out_score);
    });
    return hipGetLastError();
}

// The 64-bit inclusive scan of v[0 .. n) in place (sums: join_scan_blocks(n) words): three launches.
static void launch_join_scan(uint64_t *v, uint64_t n, uint64_t *sums, hipStream_t stream)
{
    const unsigned nb = (unsigned)join_scan_blocks(n);
    hipLaunchKernelGGL(k_join_scan_sums, dim3(nb), dim3(JOIN_SCAN_BLOCK), 0, stream, v, n, sums);
    hipLaunchKernelGGL(k_join_scan_top, dim3(1), dim3(JOIN_SCAN_BLOCK), 0, stream, sums, (uint64_t)nb);
    hipLaunchKernelGGL(k_join_scan_apply, dim3(nb), dim3(JOIN_SCAN_BLOCK), 0, stream, v, n, sums);
}

hipError_t launch_join_indptr(uint32_t *cnt, uint32_t nq, uint32_t lists, uint64_t *indptr, uint64_t *sums, hipStream_t stream)
{
    hipLaunchKernelGGL(k_join_totals, dim3(match_grid(nq)), dim3(MATCH_BLOCK), 0, stream, cnt, nq, lists, indptr);
    launch_join_scan(indptr + 1, nq, sums, stream);
    return hipGetLastError();
}

template <int SIDE>
static void launch_join_slow_side(bool fill, const JoinSlowArgs &a)
{
    const uint32_t rows = SIDE == 0 ? a.nc : a.nq;
    with_fill(fill, [&](auto FILL) {
        hipLaunchKernelGGL((k_join_slow<SIDE, decltype(FILL)::value>), dim3(match_grid(rows), a.nb), dim3(MATCH_BLOCK), 0, a.stream, a.scores, a.list,
                           a.qmeta, rows, a.cutoff, a.upper, a.fb, a.cur, a.indptr, a.out_index, a.out_score);
    });
}

hipError_t launch_join_slow(int side, bool fill, const JoinSlowArgs &a)
{
    if (a.nb == 0u || a.nq == 0u || a.nc == 0u) return hipSuccess;
    if (side == 0) launch_join_slow_side<0>(fill, a);
    else launch_join_slow_side<1>(fill, a);
    return hipGetLastError();
}

hipError_t launch_join_sort_rows(const uint64_t *indptr, uint32_t nq, uint32_t nc, uint32_t *index, double *score, hipStream_t stream)
{
    if (nq == 0u || nc < 2u) return hipSuccess;
    const uint32_t per = JOIN_SORT_BLOCK / 64u;
    hipLaunchKernelGGL(k_join_sort_rows<false>, dim3((unsigned)(((uint64_t)nq + per - 1u) / per)), dim3(JOIN_SORT_BLOCK), 0, stream, indptr, nq, index,
                       score);
    if (nc > JOIN_SORT_WAVE_MAX) // (a row has at most nc hits)
        hipLaunchKernelGGL(k_join_sort_rows<true>, dim3(nq < 4096u ? nq : 4096u), dim3(JOIN_SORT_BLOCK), 0, stream, indptr, nq, index, score);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// threshold join by the reference measures (strsim_match_join_kernels.h)
// ------------------------------------------------------------------------------------------------
template <int M>
static void launch_match_join_lane_m(bool fill, const JoinLaneArgs &a, const double *qtab, const MatchJoinNeed &need, double min_score)
{
    with_fill(fill, [&](auto FILL) {
        hipLaunchKernelGGL((k_match_join_lane<M, decltype(FILL)::value>), dim3(match_grid(a.nq), a.splits), dim3(MATCH_BLOCK), 0, a.stream, a.qwords,
                           a.qmeta, a.qperm, a.qstart, a.nq, a.swords, a.smeta, a.sidx, a.cstart, qtab, need, min_score, a.upper, a.cnt, a.map,
                           a.map_words, a.map_shift, a.indptr, a.out_index, a.out_score);
    });
}

hipError_t launch_match_join_lane(int measure, bool fill, const JoinLaneArgs &a, const double *qtab, const MatchJoinNeed &need, double min_score)
{
    switch (measure) {
    case LEVENSHTEIN: launch_match_join_lane_m<LEVENSHTEIN>(fill, a, qtab, need, min_score); break;
    case JARO: launch_match_join_lane_m<JARO>(fill, a, qtab, need, min_score); break;
    case JARO_WINKLER: launch_match_join_lane_m<JARO_WINKLER>(fill, a, qtab, need, min_score); break;
    case JACCARD: launch_match_join_lane_m<JACCARD>(fill, a, qtab, need, min_score); break;
    default: launch_match_join_lane_m<SORENSEN_DICE>(fill, a, qtab, need, min_score); break;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// connected components (strsim_components_kernels.h)
// ------------------------------------------------------------------------------------------------
static unsigned components_grid(uint32_t rows) { return (unsigned)(((uint64_t)rows + COMPONENTS_BLOCK - 1u) / COMPONENTS_BLOCK); }

hipError_t launch_components_identity(uint32_t rows, uint32_t *out_root, uint32_t *out_cluster, hipStream_t stream)
{
    hipLaunchKernelGGL(k_components_identity, dim3(components_grid(rows)), dim3(COMPONENTS_BLOCK), 0, stream, rows, out_root, out_cluster);
    return hipGetLastError();
}

hipError_t launch_components(const ComponentsArgs &a)
{
    const dim3 grid(components_grid(a.rows)), block(COMPONENTS_BLOCK);
    hipLaunchKernelGGL(k_components_init, grid, block, 0, a.stream, a.rows, a.parent, a.status);
    hipLaunchKernelGGL(k_components_link, dim3(components_link_grid(a.nnz)), block, 0, a.stream, a.indptr, a.index, a.rows, a.nnz, a.parent, a.status);
    hipLaunchKernelGGL(k_components_compress, grid, block, 0, a.stream, a.rows, a.parent, a.out_root, a.scan);
    launch_join_scan(a.scan, a.rows, a.sums, a.stream);
    hipLaunchKernelGGL(k_components_rank, grid, block, 0, a.stream, a.rows, a.out_root, a.scan, a.out_cluster, a.status);
    return hipGetLastError();
}

// OUT = uint32_t: the distance into out32; OUT = double (OSA alone): the similarity into a.out
template <bool TR, typename OUT>
static void launch_dist_lane_as(const LaunchArgs &a, uint32_t k, OUT *out, uint32_t *worklist)
{
    with_literal(a, [&](auto LIT) {
        hipLaunchKernelGGL((k_dist_lane<TR, decltype(LIT)::value, OUT>), lane_grid(a), dim3(256), 0, a.stream, a.offA, a.valA, a.offB, a.valB, a.n,
                           k, out, worklist, a.status);
    });
}

template <bool TR, typename OUT>
static void launch_dist_wave_as(const LaunchArgs &a, uint32_t k, OUT *out, const uint32_t *worklist, int grid, uint32_t *scratch,
                                uint64_t slot_words)
{
    hipLaunchKernelGGL((k_dist_wave<TR, OUT>), dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB, a.rowsB,
                       k, out, worklist, a.status, scratch, slot_words);
}

hipError_t launch_dist_lane(int measure, const LaunchArgs &a, uint32_t k, uint32_t *out32, uint32_t *worklist)
{
    if (measure != OSA) launch_dist_lane_as<false>(a, k, out32, worklist);
    else if (out32) launch_dist_lane_as<true>(a, k, out32, worklist);
    else launch_dist_lane_as<true>(a, k, a.out, worklist);
    return hipGetLastError();
}

hipError_t launch_dist_wave(int measure, const LaunchArgs &a, uint32_t k, uint32_t *out32, const uint32_t *worklist, int grid,
                            uint32_t *scratch, uint64_t slot_words)
{
    if (measure != OSA) launch_dist_wave_as<false>(a, k, out32, worklist, grid, scratch, slot_words);
    else if (out32) launch_dist_wave_as<true>(a, k, out32, worklist, grid, scratch, slot_words);
    else launch_dist_wave_as<true>(a, k, a.out, worklist, grid, scratch, slot_words);
    return hipGetLastError();
}

hipError_t launch_indel_lane(const LaunchArgs &a, uint32_t k, uint32_t *out32, uint32_t *worklist)
{
    with_literal(a, [&](auto LIT) {
        hipLaunchKernelGGL(k_indel_lane<decltype(LIT)::value>, lane_grid(a), dim3(256), 0, a.stream, a.offA, a.valA, a.offB, a.valB, a.n, k, a.out,
                           out32, worklist, a.status);
    });
    return hipGetLastError();
}

hipError_t launch_indel_wave(const LaunchArgs &a, uint32_t k, uint32_t *out32, const uint32_t *worklist, int grid, uint32_t *scratch,
                             uint64_t slot_words)
{
    hipLaunchKernelGGL(k_indel_wave, dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB, a.rowsB, k,
                       a.out, out32, worklist, a.status, scratch, slot_words);
    return hipGetLastError();
}

// OUT = uint32_t: the distance into out32; OUT = double: the similarity into a.out
template <typename OUT>
static void launch_dl_lane_as(const LaunchArgs &a, uint32_t k, OUT *out, uint32_t *worklist)
{
    with_literal(a, [&](auto LIT) {
        hipLaunchKernelGGL((k_dl_lane<decltype(LIT)::value, OUT>), lane_grid(a), dim3(256), 0, a.stream, a.offA, a.valA, a.offB, a.valB, a.n, k,
                           out, worklist, a.status);
    });
}

template <typename OUT>
static void launch_dl_wave_as(const LaunchArgs &a, uint32_t k, OUT *out, uint64_t cols, const uint32_t *worklist, int grid, uint32_t *scratch,
                              uint64_t slot_words)
{
    if (cols <= DL_WAVE_SMALL_COLS)
        hipLaunchKernelGGL((k_dl_wave<DL_WAVE_SMALL_COLS, OUT>), dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB,
                           a.valB, a.rowsB, k, out, worklist, a.status, scratch, slot_words);
    else
        hipLaunchKernelGGL((k_dl_wave<DL_WAVE_LDS_COLS, OUT>), dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB,
                           a.valB, a.rowsB, k, out, worklist, a.status, scratch, slot_words);
}

hipError_t launch_dl_lane(const LaunchArgs &a, uint32_t k, uint32_t *out32, uint32_t *worklist)
{
    if (out32) launch_dl_lane_as(a, k, out32, worklist);
    else launch_dl_lane_as(a, k, a.out, worklist);
    return hipGetLastError();
}

hipError_t launch_dl_wave(const LaunchArgs &a, uint32_t k, uint32_t *out32, uint64_t cols, const uint32_t *worklist, int grid, uint32_t *scratch,
                          uint64_t slot_words)
{
    if (out32) launch_dl_wave_as(a, k, out32, cols, worklist, grid, scratch, slot_words);
    else launch_dl_wave_as(a, k, a.out, cols, worklist, grid, scratch, slot_words);
    return hipGetLastError();
}

// f(std::integral_constant<int, MODE>): the output of a strsim_common call
template <class F>
static void with_common_out(int mode, F f)
{
    if (mode == COMMON_OUT_SIM) f(std::integral_constant<int, COMMON_OUT_SIM>{});
    else if (mode == COMMON_OUT_DIST) f(std::integral_constant<int, COMMON_OUT_DIST>{});
    else f(std::integral_constant<int, COMMON_OUT_COUNT>{});
}

template <int KIND>
static void launch_common_lane_as(const LaunchArgs &a, int mode, uint32_t k, void *out, uint32_t *worklist)
{
    with_common_out(mode, [&](auto OUT) {
        with_literal(a, [&](auto LIT) {
            hipLaunchKernelGGL((k_common_lane<KIND, decltype(LIT)::value, decltype(OUT)::value>), lane_grid(a), dim3(256), 0, a.stream, a.offA,
                               a.valA, a.offB, a.valB, a.n, k, out, worklist, a.status);
        });
    });
}

template <int KIND>
static void launch_common_wave_as(const LaunchArgs &a, int mode, uint32_t k, void *out, const uint32_t *worklist, int grid)
{
    with_common_out(mode, [&](auto OUT) {
        hipLaunchKernelGGL((k_common_wave<KIND, decltype(OUT)::value>), dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA,
                           a.offB, a.valB, a.rowsB, k, out, worklist, a.status);
    });
}

hipError_t launch_common_lane(const LaunchArgs &a, int kind, int mode, uint32_t k, void *out, uint32_t *worklist)
{
    if (mode != COMMON_OUT_DIST) k = DIST_UNBOUNDED;
    switch (kind) {
    case COMMON_HAMMING: launch_common_lane_as<COMMON_HAMMING>(a, mode, k, out, worklist); break;
    case COMMON_PREFIX: launch_common_lane_as<COMMON_PREFIX>(a, mode, k, out, worklist); break;
    case COMMON_POSTFIX: launch_common_lane_as<COMMON_POSTFIX>(a, mode, k, out, worklist); break;
    default:
        with_literal(a, [&](auto LIT) {
            hipLaunchKernelGGL(k_common_lcs_lane<decltype(LIT)::value>, lane_grid(a), dim3(256), 0, a.stream, a.offA, a.valA, a.offB, a.valB, a.n,
                               k, mode, out, worklist, a.status);
        });
    }
    return hipGetLastError();
}

hipError_t launch_common_wave(const LaunchArgs &a, int kind, int mode, uint32_t k, void *out, const uint32_t *worklist, int grid,
                              uint32_t *scratch, uint64_t slot_words)
{
    if (mode != COMMON_OUT_DIST) k = DIST_UNBOUNDED;
    switch (kind) {
    case COMMON_HAMMING: launch_common_wave_as<COMMON_HAMMING>(a, mode, k, out, worklist, grid); break;
    case COMMON_PREFIX: launch_common_wave_as<COMMON_PREFIX>(a, mode, k, out, worklist, grid); break;
    case COMMON_POSTFIX: launch_common_wave_as<COMMON_POSTFIX>(a, mode, k, out, worklist, grid); break;
    default:
        hipLaunchKernelGGL(k_common_lcs_wave, dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB, a.rowsB, k,
                           mode, out, worklist, a.status, scratch, slot_words);
    }
    return hipGetLastError();
}

// f(std::integral_constant<int, Q>, std::bool_constant<SET>): the q (1..3) and the mode of a q-gram call
template <class F>
static void with_qgram(uint32_t q, bool set, F f)
{
    auto mode = [&](auto Q) {
        if (set) f(Q, std::true_type{});
        else f(Q, std::false_type{});
    };
    if (q == 1u) mode(std::integral_constant<int, 1>{});
    else if (q == 2u) mode(std::integral_constant<int, 2>{});
    else mode(std::integral_constant<int, 3>{});
}

hipError_t launch_qgram_lane(const LaunchArgs &a, int kind, uint32_t q, bool set, uint32_t *worklist)
{
    with_qgram(q, set, [&](auto Q, auto SET) {
        hipLaunchKernelGGL((k_qgram_lane<decltype(Q)::value, decltype(SET)::value>), lane_grid(a), dim3(256), 0, a.stream, a.offA, a.valA, a.rowsA,
                           a.offB, a.valB, a.rowsB, a.n, kind, a.out, worklist, a.status);
    });
    return hipGetLastError();
}

hipError_t launch_qgram_wave(const LaunchArgs &a, int kind, uint32_t q, bool set, uint64_t grams, const uint32_t *worklist, int grid,
                             uint32_t *scratch, uint64_t slot_words)
{
    const uint64_t slots = qgram_table_slots(grams); // (the layout of a scratch slot: qgram_wave_slot_words)
    with_qgram(q, set, [&](auto Q, auto SET) {
        if (grams <= QGRAM_WAVE_SMALL_GRAMS)
            hipLaunchKernelGGL((k_qgram_wave<QGRAM_WAVE_SMALL_GRAMS, decltype(Q)::value, decltype(SET)::value>), dim3((unsigned)grid), dim3(64), 0,
                               a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB, a.rowsB, kind, a.out, worklist, a.status, scratch, slot_words, slots);
        else
            hipLaunchKernelGGL((k_qgram_wave<QGRAM_WAVE_LDS_GRAMS, decltype(Q)::value, decltype(SET)::value>), dim3((unsigned)grid), dim3(64), 0,
                               a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB, a.rowsB, kind, a.out, worklist, a.status, scratch, slot_words, slots);
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// threshold join by q-gram similarity (strsim_qgram_join_kernels.h)
// ------------------------------------------------------------------------------------------------
hipError_t launch_qgram_join_first(uint32_t q, const JoinLaneArgs &a, uint32_t nc, uint32_t *first)
{
    with_qgram(q, true, [&](auto Q, auto) {
        hipLaunchKernelGGL(k_qgram_join_first<decltype(Q)::value>, dim3(match_grid(nc)), dim3(MATCH_BLOCK), 0, a.stream, a.swords, a.smeta, a.cstart,
                           nc, first);
    });
    return hipGetLastError();
}

hipError_t launch_qgram_join_lane(int kind, uint32_t q, bool set, bool fill, const JoinLaneArgs &a, const uint32_t *first, const MatchJoinNeed &need,
                                  double min_score)
{
    with_qgram(q, set, [&](auto Q, auto SET) {
        with_fill(fill, [&](auto FILL) {
            hipLaunchKernelGGL((k_qgram_join_lane<decltype(Q)::value, decltype(SET)::value, decltype(FILL)::value>), dim3(match_grid(a.nq), a.splits),
                               dim3(MATCH_BLOCK), 0, a.stream, a.qwords, a.qmeta, a.qperm, a.qstart, a.nq, a.swords, a.smeta, a.sidx, a.cstart, kind,
                               first, need, min_score, a.upper, a.cnt, a.map, a.map_words, a.map_shift, a.indptr, a.out_index, a.out_score);
        });
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// join by integer edit distance (strsim_distance_join_kernels.h)
// ------------------------------------------------------------------------------------------------
template <int KIND>
static void launch_distance_join_lane_k(bool fill, const JoinLaneArgs &a, const MatchJoinNeed &need, uint32_t max_distance)
{
    with_fill(fill, [&](auto FILL) {
        hipLaunchKernelGGL((k_distance_join_lane<KIND, decltype(FILL)::value>), dim3(match_grid(a.nq), a.splits), dim3(MATCH_BLOCK), 0, a.stream,
                           a.qwords, a.qmeta, a.qperm, a.qstart, a.nq, a.swords, a.smeta, a.sidx, a.cstart, need, max_distance, a.upper, a.cnt, a.map,
                           a.map_words, a.map_shift, a.indptr, a.out_index, a.out_score);
    });
}

hipError_t launch_distance_join_lane(int kind, bool fill, const JoinLaneArgs &a, const MatchJoinNeed &need, uint32_t max_distance)
{
    switch (kind) {
    case EDIT_LEVENSHTEIN: launch_distance_join_lane_k<EDIT_LEVENSHTEIN>(fill, a, need, max_distance); break;
    case EDIT_OSA: launch_distance_join_lane_k<EDIT_OSA>(fill, a, need, max_distance); break;
    default: launch_distance_join_lane_k<EDIT_DAMERAU>(fill, a, need, max_distance); break;
    }
    return hipGetLastError();
}

hipError_t launch_distance_join_finish(const double *score, uint64_t n, uint32_t *dist, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_distance_join_finish, dim3(match_grid(n)), dim3(MATCH_BLOCK), 0, stream, score, n, dist);
    return hipGetLastError();
}

template <bool ALIGN>
static void launch_partial_lane_al(const LaunchArgs &a, uint32_t *span, uint32_t *worklist)
{
    with_literal(a, [&](auto LIT) {
        hipLaunchKernelGGL((k_partial_lane<decltype(LIT)::value, ALIGN>), lane_grid(a), dim3(256), 0, a.stream, a.offA, a.valA, a.offB, a.valB, a.n,
                           a.out, span, worklist, a.status);
    });
}

hipError_t launch_partial_lane(const LaunchArgs &a, uint32_t *span, uint32_t *worklist)
{
    if (span) launch_partial_lane_al<true>(a, span, worklist);
    else launch_partial_lane_al<false>(a, span, worklist);
    return hipGetLastError();
}

hipError_t launch_partial_wave(const LaunchArgs &a, uint32_t *span, const uint32_t *worklist, int grid, uint32_t *scratch, uint64_t slot_words)
{
    if (span)
        hipLaunchKernelGGL(k_partial_wave<true>, dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB,
                           a.rowsB, a.out, span, worklist, a.status, scratch, slot_words);
    else
        hipLaunchKernelGGL(k_partial_wave<false>, dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB,
                           a.rowsB, a.out, span, worklist, a.status, scratch, slot_words);
    return hipGetLastError();
}

hipError_t launch_token_bounds(const uint32_t *off, uint64_t rows, TokenStatus *st, int side, hipStream_t stream)
{
    const uint64_t blocks = (rows + 255u) / 256u;
    hipLaunchKernelGGL(k_token_bounds, dim3((unsigned)(blocks < 4096u ? blocks : 4096u)), dim3(256), 0, stream, off, rows, st, side);
    return hipGetLastError();
}

hipError_t launch_token_sort(bool write, const uint32_t *off, const uint8_t *val, uint64_t rows, uint32_t *out_off, uint8_t *out_val,
                             uint32_t *list, uint32_t *count, int grid, uint32_t *scratch, uint64_t slot_words, hipStream_t stream)
{
    const dim3 lane_grid((unsigned)((rows + 255u) / 256u));
    if (write) {
        hipLaunchKernelGGL(k_token_sort_lane<true>, lane_grid, dim3(256), 0, stream, off, val, rows, out_off, out_val, list, count);
        hipLaunchKernelGGL(k_token_sort_wave<true>, dim3((unsigned)grid), dim3(64), 0, stream, off, val, out_off, out_val, list, count, scratch, slot_words);
    } else {
        hipLaunchKernelGGL(k_token_sort_lane<false>, lane_grid, dim3(256), 0, stream, off, val, rows, out_off, out_val, list, count);
        hipLaunchKernelGGL(k_token_sort_wave<false>, dim3((unsigned)grid), dim3(64), 0, stream, off, val, out_off, out_val, list, count, scratch, slot_words);
    }
    return hipGetLastError();
}

hipError_t launch_token_set(bool write, const LaunchArgs &a, uint32_t *off_ab, uint8_t *val_ab, uint32_t *off_ba, uint8_t *val_ba,
                            TokenSetRec *rec, uint32_t *list, uint32_t *count, int grid, uint32_t *scratch, uint64_t slot_words)
{
    const dim3 lane_grid((unsigned)((a.n + 255u) / 256u));
    if (write) {
        hipLaunchKernelGGL(k_token_set_lane<true>, lane_grid, dim3(256), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB, a.rowsB, a.n,
                           off_ab, val_ab, off_ba, val_ba, rec, list, count);
        hipLaunchKernelGGL(k_token_set_wave<true>, dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB, a.rowsB,
                           off_ab, val_ab, off_ba, val_ba, rec, list, count, scratch, slot_words);
    } else {
        hipLaunchKernelGGL(k_token_set_lane<false>, lane_grid, dim3(256), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB, a.rowsB, a.n,
                           off_ab, val_ab, off_ba, val_ba, rec, list, count);
        hipLaunchKernelGGL(k_token_set_wave<false>, dim3((unsigned)grid), dim3(64), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB, a.rowsB,
                           off_ab, val_ab, off_ba, val_ba, rec, list, count, scratch, slot_words);
    }
    return hipGetLastError();
}

hipError_t launch_token_scan(uint32_t *out_off, uint64_t rows, uint32_t *sums, hipStream_t stream)
{
    const unsigned nb = (unsigned)((rows + TOKEN_SCAN_BLOCK - 1u) / TOKEN_SCAN_BLOCK);
    hipLaunchKernelGGL(k_token_scan_sums, dim3(nb), dim3(256), 0, stream, out_off + 1, rows, sums);
    hipLaunchKernelGGL(k_token_scan_top, dim3(1), dim3(256), 0, stream, sums, nb);
    hipLaunchKernelGGL(k_token_scan_apply, dim3(nb), dim3(256), 0, stream, out_off + 1, rows, sums);
    return hipGetLastError();
}

hipError_t launch_process(bool write, const uint32_t *off, const uint8_t *val, uint64_t rows, uint32_t *out_off, uint8_t *out_val, uint32_t *list,
                          uint32_t *count, int grid, const ProcessTable &t, hipStream_t stream)
{
    const dim3 lane_grid((unsigned)((rows + 255u) / 256u));
    if (write) {
        hipLaunchKernelGGL(k_process_lane<true>, lane_grid, dim3(256), 0, stream, off, val, rows, out_off, out_val, list, count);
        hipLaunchKernelGGL(k_process_wave<true>, dim3((unsigned)grid), dim3(64), 0, stream, off, val, out_off, out_val, list, count, t);
    } else {
        hipLaunchKernelGGL(k_process_lane<false>, lane_grid, dim3(256), 0, stream, off, val, rows, out_off, out_val, list, count);
        hipLaunchKernelGGL(k_process_wave<false>, dim3((unsigned)grid), dim3(64), 0, stream, off, val, out_off, out_val, list, count, t);
    }
    return hipGetLastError();
}

hipError_t launch_token_set_epilogue(const TokenSetRec *rec, const uint32_t *d32, double *out, uint64_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_token_set_epilogue, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, rec, d32, out, n);
    return hipGetLastError();
}

hipError_t launch_wratio_classify(const LaunchArgs &a, uint8_t *cls, uint32_t *pos, uint32_t *list_near, uint32_t *list_far, WratioStatus *st)
{
    hipLaunchKernelGGL(k_wratio_classify, dim3((unsigned)((a.n + 255u) / 256u)), dim3(256), 0, a.stream, a.offA, a.valA, a.rowsA, a.offB, a.valB,
                       a.rowsB, a.n, cls, pos, list_near, list_far, st);
    return hipGetLastError();
}

hipError_t launch_take(const uint32_t *off, const uint8_t *val, const uint32_t *list, uint32_t m, uint32_t *out_off, uint8_t *out_val,
                       uint32_t *sums, hipStream_t stream)
{
    hipLaunchKernelGGL(k_take_measure, dim3((unsigned)(((uint64_t)m + 255u) / 256u)), dim3(256), 0, stream, off, list, m, out_off);
    hipError_t e = launch_token_scan(out_off, m, sums, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_take_write, dim3((unsigned)(((uint64_t)m * TAKE_LANES + 255u) / 256u)), dim3(256), 0, stream, off, val, list, m, out_off,
                       out_val);
    return hipGetLastError();
}

hipError_t launch_wratio_combine(const LaunchArgs &a, const uint8_t *cls, const uint32_t *pos, const double *s_near, const double *s_far0,
                                 const double *s_far1)
{
    hipLaunchKernelGGL(k_wratio_combine, dim3((unsigned)((a.n + 255u) / 256u)), dim3(256), 0, a.stream, cls, pos, s_near, s_far0, s_far1, a.out, a.n);
    return hipGetLastError();
}

hipError_t launch_max_f64(const double *x, const double *y, double *out, uint64_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_max_f64, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, x, y, out, n);
    return hipGetLastError();
}

hipError_t launch_partial_token_set_epilogue(const TokenSetRec *rec, const double *p, double *out, uint64_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_partial_token_set_epilogue, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, rec, p, out, n);
    return hipGetLastError();
}

} // namespace strsim


#if STRSIM_BOUNDS_ON
// lab build only (EXTRA="-DSTRSIM_LAB -DSTRSIM_BOUNDS"): the address-check record of this translation unit's kernels -> dst[0..5]
// (hits, kernel << 32 | site, row, value, lo, hi), and cleared.  Call after the stream has been synchronised.
extern "C" __attribute__((visibility("default"))) int strsim_debug_bounds_kernels(unsigned long long *dst)
{
    strsim::bounds::Record r{};
    hipError_t e = hipMemcpyFromSymbol(&r, HIP_SYMBOL(strsim::bounds::g_rec), sizeof(r), 0, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    dst[0] = r.hits; dst[1] = r.site; dst[2] = r.row; dst[3] = r.value; dst[4] = r.lo; dst[5] = r.hi;
    const strsim::bounds::Record z{};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(strsim::bounds::g_rec), &z, sizeof(z), 0, hipMemcpyHostToDevice);
}
#endif

#if defined(STRSIM_LAB) && defined(STRSIM_WIDE_STAMPS)
// lab build only: copies the per-wave phase cycle sums of the last k_lane_wide launch to the host
extern "C" __attribute__((visibility("default"))) int strsim_debug_wide_stamps(unsigned long long *dst, size_t waves)
{
    if (waves > 16384) waves = 16384;
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(strsim::g_wide_stamps), waves * 16 * sizeof(unsigned long long), 0,
                                    hipMemcpyDeviceToHost);
}
#endif

#if defined(STRSIM_LAB) && defined(STRSIM_STAGE_STAMPS)
// lab build only: copies the per-wave phase cycle sums of the last k_lane_stage launch to the host
extern "C" __attribute__((visibility("default"))) int strsim_debug_stage_stamps(unsigned long long *dst, size_t waves)
{
    if (waves > 16384) waves = 16384;
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(strsim::g_stage_stamps), waves * 16 * sizeof(unsigned long long), 0,
                                    hipMemcpyDeviceToHost);
}
#endif
