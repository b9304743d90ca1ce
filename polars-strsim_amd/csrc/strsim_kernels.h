// strsim_kernels.h -- launch interface between the C ABI (strsim_capi.cpp) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "strsim_lane_core.h" // QTAB_N

namespace strsim {

constexpr int WAVE_CAP = 1024; // wave-per-pair kernels: max bytes (hence scalar values) per string

// k_wave_pairs<LEVENSHTEIN>: up to LEV_JOBS pairs are advanced together by one wave.  Its per-wave global scratch: the
// three scalar-value arrays of the fallback, then the text arena of a BYTES batch (ASCII texts as bytes), the text
// arena of a SYMBOLS batch (16-bit scalar values) and the SYMBOLS patterns (32 values per lane); a staged text has
// TXT_PAD units in front of and behind it.
#ifndef STRSIM_LEV_JOBS
#define STRSIM_LEV_JOBS 16
#endif
constexpr int LEV_JOBS = STRSIM_LEV_JOBS;
#ifndef STRSIM_LEV_POOL
#define STRSIM_LEV_POOL 384 // rows ranked together before they are dealt into batches, at most (a multiple of 64; 16 bits of LDS per row)
#endif
constexpr int LEV_POOL = STRSIM_LEV_POOL;
constexpr int TXT_PAD = 48;
constexpr int ARENA0_BYTES = 8192;
constexpr int ARENA1_BYTES = 12288;
constexpr int PAT1_BYTES = 64 * 32 * 2;
constexpr int LEV_WS_WORDS = 3 * (WAVE_CAP + 64) + (ARENA0_BYTES + ARENA1_BYTES + PAT1_BYTES) / 4; // per wave

// k_huge_pairs: words of global workspace per wave for strings of up to `cap` bytes: a front pad, the two arrays of
// scalar values, and an auxiliary array four times as long (hash table of the multiset intersection: 2 (cap + 64)
// 64-bit entries; Jaro flags; Levenshtein hand-off bytes)
#define HUGE_WS_WORDS(cap) (6u * ((uint64_t)(cap) + 64u) + 64u)

struct DevStatus {
    unsigned int wave_rows; // rows finished by k_wave_pairs
    unsigned int huge_rows; // rows longer than WAVE_CAP (left for the long-string pass)
    unsigned int max_len;   // longest such string, bytes
    unsigned int lane_left; // rows the one-pair-per-lane kernel left to the kernels behind it (written for eager calls only)
    // per measure (the fused five-measure call runs the slow-row kernels once per measure):
    unsigned int list_count[5]; // k_lane_utf8: chunks of 64 rows that still hold unfinished rows ...
    unsigned int list_rows[5];  // ... and how many rows that is
    unsigned int next_entry[5]; // k_wave_pairs: work-list entries handed out beyond the first static round
    unsigned int pad1[12];
    unsigned int ticket;    // host-mapped copy only: the call's ticket, written LAST (release, system scope) by whoever publishes
                            // the block -- strsim_ctx_retire_oldest() refuses a slot whose ticket has not arrived
};
static_assert(sizeof(DevStatus) == 128, "DevStatus is 128 bytes");

struct LaunchArgs {
    const uint32_t *offA; const uint8_t *valA; uint64_t rowsA;
    const uint32_t *offB; const uint8_t *valB; uint64_t rowsB;
    double *out; uint64_t n;
    unsigned long long *slowmask; // one 64-bit mask per 64-row chunk
    uint32_t *worklist;           // ceil(n/64) words: the non-empty chunks, compacted by k_lane_utf8
    const double *qtab;           // QTAB_N x QTAB_N integer quotients a / b for the epilogues of the one-pair-per-lane kernels (device)
    DevStatus *status;            // cleared by the first kernel of the call
    uint32_t *sched;              // k_lane_stage: four zeroed words (range counter, finished workgroups, rows left, -); left zeroed by the kernel
    DevStatus *publish_host;      // the last workgroup of k_lane_stage writes lane_left there (host-mapped), else nullptr
    uint32_t publish_ticket;      // != 0: ... and then this ticket: the call consists of that kernel alone
    hipStream_t stream;
    int wide_grid, wave_grid;     // resident workgroups of k_lane_wide / k_lane_utf8, waves of k_wave_pairs
    bool no_literal_path;         // A/B runs: a literal call takes k_lane_stage like any other
    bool long_rows;               // the context's last call left many rows behind k_lane_stage: take its instantiation without tables
    int stage_grid;               // k_lane_stage: persistent workgroups at STRSIM_STAGE_WAVES_PER_EU per CU
    int wide_grid_cap;            // k_lane_wide / k_lane_utf8: launch size limit (wide_grid = what is resident)
    int wave_grid_lev;            // k_wave_pairs<LEVENSHTEIN> (LDS-light: more waves per CU)
    uint32_t *lev_ws;             // its global scratch: wave_grid_lev * LEV_WS_WORDS words
    hipEvent_t ev_lane0, ev_lane1, ev_wave1; // optional (nullptr = no timing)
};

hipError_t launch_pairs(int measure, const LaunchArgs &a);
// the two halves of launch_pairs for a call that looks at lane_left in between (small calls: usually nothing is left)
hipError_t launch_lane_only(int measure, const LaunchArgs &a);
hipError_t launch_slow_only(int measure, const LaunchArgs &a);
// the same two halves of launch_pairs_all
hipError_t launch_lane_all_only(const LaunchArgs &a, double *const outs[5]);
hipError_t launch_slow_all_only(const LaunchArgs &a, double *const outs[5], unsigned long long *mask_backup);
// (every first kernel of a call -- k_lane_stage, k_lane_stage_all, k_lane_lit + k_publish_lit -- reports lane_left and the ticket)
// launches the first kernel of such a call takes: 1, or 2 when a literal takes k_lane_lit (+ k_publish_lit behind it)
int lane_kernel_launches(int measure, const LaunchArgs &a);
int wave_lev_resident_per_cu();

// All five measures in one go (a.out unused): outs[] indexed by measure id; mask_backup = ceil(n/64) words of scratch.
hipError_t launch_pairs_all(const LaunchArgs &a, double *const outs[5], unsigned long long *mask_backup);

// Second pass for rows with a string longer than WAVE_CAP bytes: `grid` waves, each with HUGE_WS_WORDS(cap) words of `ws`.
hipError_t launch_huge(int measure, const LaunchArgs &a, uint32_t *ws, uint32_t cap, int grid);
// copies one DevStatus to host-mapped pinned memory from the device side (no copy-engine hand-over)
hipError_t launch_publish_status(const DevStatus *src, DevStatus *dst_mapped, uint32_t ticket, hipStream_t stream);

// Best match (strsim_match.h).  The lane kernel's top-K is instantiated at K = 1, 4, 16: match_lane_k(k) is the K a call with k
// slots runs at (its lists are K long; the merge writes the first k).
int match_lane_k(uint32_t k);
struct MatchLaneArgs {
    const uint32_t *qwords, *qmeta; uint32_t nq; // queries: eight words + meta per string (k_match_pack)
    const uint32_t *cwords, *cmeta; uint32_t nc; // candidates
    uint32_t splits, per;                         // grid.y and candidates per split
    uint32_t k;
    const double *qtab;
    double min_score;
    double *pscore; uint32_t *pidx;               // splits x nq x match_lane_k(k) partial lists
    hipStream_t stream;
};
hipError_t launch_match_pack(const uint32_t *off, const uint8_t *val, uint32_t rows, uint32_t *words, uint32_t *meta,
                             uint32_t *slow_list, uint32_t *slow_count, hipStream_t stream);
hipError_t launch_match_lane(int measure, const MatchLaneArgs &a);
hipError_t launch_match_clear(double *score, uint32_t *idx, uint64_t n, hipStream_t stream);
hipError_t launch_match_fold_cols(uint32_t k, const double *scores, const uint32_t *qlist, uint32_t nb, uint32_t nc, double min_score,
                                  double *fscore, uint32_t *fidx, hipStream_t stream);
hipError_t launch_match_fold_rows(uint32_t k, const double *scores, const uint32_t *clist, uint32_t nb, const uint32_t *qmeta, uint32_t nq,
                                  double min_score, double *fscore, uint32_t *fidx, hipStream_t stream);
hipError_t launch_match_merge(uint32_t k, const double *pscore, const uint32_t *pidx, uint32_t nl, uint32_t nq, uint32_t *out_index,
                              double *out_score, hipStream_t stream);

// Edit distances (strsim_distance.h): measure 0 (Levenshtein) or 6 (OSA).  k_dist_lane over all a.n rows: the rows it cannot take
// go to `worklist` (a.n words), counted in a.status->wave_rows, with a.status->max_len a bound of their pattern lengths; the caller
// zeroes the status block first.  k_dist_wave then finishes the work list on `grid` waves, each with slot_words words of `scratch`
// (patterns longer than OSA_WAVE_LDS_CPS scalar values; nullptr when there are none).  out32 != nullptr: the uint32 distance
// clamped by k into out32 (a.out is not used); out32 == nullptr, measure 6 alone: the f64 OSA similarity into a.out
// (k = DIST_UNBOUNDED).
hipError_t launch_dist_lane(int measure, const LaunchArgs &a, uint32_t k, uint32_t *out32, uint32_t *worklist);
hipError_t launch_dist_wave(int measure, const LaunchArgs &a, uint32_t k, uint32_t *out32, const uint32_t *worklist, int grid,
                            uint32_t *scratch, uint64_t slot_words);

// Indel similarity / distance (strsim_indel.h), measure id 8: the same two-kernel protocol.  out32 == nullptr: the f64 similarity
// into a.out (k = DIST_UNBOUNDED); otherwise the uint32 distance clamped by k into out32 (a.out is not used).
hipError_t launch_indel_lane(const LaunchArgs &a, uint32_t k, uint32_t *out32, uint32_t *worklist);
hipError_t launch_indel_wave(const LaunchArgs &a, uint32_t k, uint32_t *out32, const uint32_t *worklist, int grid, uint32_t *scratch,
                             uint64_t slot_words);

// Partial ratio (strsim_partial.h), measure id 10: the same two-kernel protocol.  The f64 score goes into a.out; span != nullptr
// adds the alignment (four uint32 per row).  k_partial_lane also leaves a bound of the work list's haystacks (bytes) in
// a.status->pad1[0]; slot_words (even) comes from partial_wave_words() of the two bounds.
hipError_t launch_partial_lane(const LaunchArgs &a, uint32_t *span, uint32_t *worklist);
hipError_t launch_partial_wave(const LaunchArgs &a, uint32_t *span, const uint32_t *worklist, int grid, uint32_t *scratch,
                               uint64_t slot_words);

// q-gram similarity (strsim_qgram.h): the same two-kernel protocol.  kind: STRSIM_QGRAM_*, q: 1..3, set: the set mode.
// k_qgram_lane leaves bounds of the work list's shorter and longer strings (bytes) in a.status->max_len and a.status->pad1[0];
// grams: their sum, a bound of the grams of a listed pair, which picks the wave kernel's LDS table and lays out a scratch slot
// (slot_words = qgram_wave_slot_words(grams, pad1[0]), for pairs of more than QGRAM_WAVE_LDS_GRAMS grams; nullptr without any).
hipError_t launch_qgram_lane(const LaunchArgs &a, int kind, uint32_t q, bool set, uint32_t *worklist);
hipError_t launch_qgram_wave(const LaunchArgs &a, int kind, uint32_t q, bool set, uint64_t grams, const uint32_t *worklist, int grid,
                             uint32_t *scratch, uint64_t slot_words);

// Unrestricted Damerau-Levenshtein similarity / distance (strsim_damerau.h): the same two-kernel protocol.  out32 == nullptr: the
// f64 similarity into a.out (k is not looked at).  k_dl_lane leaves a bound of the work list's shorter strings (bytes) in
// a.status->max_len; cols: that bound, which picks the wave kernel's LDS boundary row and lays out a scratch slot (slot_words =
// dl_wave_slot_words(cols), for pairs of more than DL_WAVE_LDS_COLS columns; nullptr without any).
hipError_t launch_dl_lane(const LaunchArgs &a, uint32_t k, uint32_t *out32, uint32_t *worklist);
hipError_t launch_dl_wave(const LaunchArgs &a, uint32_t k, uint32_t *out32, uint64_t cols, const uint32_t *worklist, int grid, uint32_t *scratch,
                          uint64_t slot_words);

// Hamming, prefix, postfix and LCSseq (strsim_common.h): the same two-kernel protocol.  kind: a CommonKind; mode: a CommonOut, which
// says what `out` holds (f64 similarity, uint32 distance under the cutoff k, uint32 count; k is looked at for the distance alone).
// Only COMMON_LCSSEQ's wave kernel takes scratch (slot_words = indel_wave_slot_words of a.status->max_len beyond OSA_WAVE_LDS_CPS).
hipError_t launch_common_lane(const LaunchArgs &a, int kind, int mode, uint32_t k, void *out, uint32_t *worklist);
hipError_t launch_common_wave(const LaunchArgs &a, int kind, int mode, uint32_t k, void *out, const uint32_t *worklist, int grid,
                              uint32_t *scratch, uint64_t slot_words);

// Token transforms (strsim_token.h), measure ids 14 and 16.  launch_token_bounds leaves a column's longest row and its first and
// last offset in st (side 0 or 1; max_len zeroed first).  A form is a measuring pass (write = false: the bytes of row i into
// out_off[i + 1], out_off[0] = 0, the rows the lane kernel cannot take onto `list`, counted in *count, zeroed first), then
// launch_token_scan over out_off (sums: ceil(rows / 4096) words), then the writing pass (write = true) with the same list.  Each
// pass is the lane kernel over every row and the wave kernel over the list on `grid` waves with slot_words words of `scratch` each
// (rows that can hold more than TOKEN_WAVE_LDS_TOKENS tokens; nullptr when there are none).
struct TokenStatus;
struct TokenSetRec;
hipError_t launch_token_bounds(const uint32_t *off, uint64_t rows, TokenStatus *st, int side, hipStream_t stream);
hipError_t launch_token_sort(bool write, const uint32_t *off, const uint8_t *val, uint64_t rows, uint32_t *out_off, uint8_t *out_val,
                             uint32_t *list, uint32_t *count, int grid, uint32_t *scratch, uint64_t slot_words, hipStream_t stream);
// the set form of a.n pairs (a.rowsA / a.rowsB == 1: a literal): ab into (off_ab, val_ab), ba into (off_ba, val_ba), one record a row
hipError_t launch_token_set(bool write, const LaunchArgs &a, uint32_t *off_ab, uint8_t *val_ab, uint32_t *off_ba, uint8_t *val_ba,
                            TokenSetRec *rec, uint32_t *list, uint32_t *count, int grid, uint32_t *scratch, uint64_t slot_words);
hipError_t launch_token_scan(uint32_t *out_off, uint64_t rows, uint32_t *sums, hipStream_t stream);
// out[i] = the rule of token_set_ratio over rec[i] and d32[i] = indel_distance(ab, ba)
hipError_t launch_token_set_epilogue(const TokenSetRec *rec, const uint32_t *d32, double *out, uint64_t n, hipStream_t stream);

// default_process (strsim_process.h): the passes of the column transform, as launch_token_sort's -- measuring (write = false), then
// launch_token_scan over out_off, then writing (write = true) with the same list; t holds device pointers of the table.
struct ProcessTable;
hipError_t launch_process(bool write, const uint32_t *off, const uint8_t *val, uint64_t rows, uint32_t *out_off, uint8_t *out_val, uint32_t *list,
                          uint32_t *count, int grid, const ProcessTable &t, hipStream_t stream);

// WRatio and the token compositions (strsim_wratio.h), measure ids 18 .. 26.  launch_wratio_classify: the class of each of a.n
// pairs into cls, its position on the near or the far list into pos, the lists counted in st->rows (zeroed first).  launch_take: the
// m rows `list` names of the column (off, val) as a column of their own -- lengths, launch_token_scan (sums: ceil(m / 4096) words),
// copy; out_val holds the column's byte size.  launch_wratio_combine: a.out holds indel(a, b) and receives the rule's result.
struct WratioStatus;
hipError_t launch_wratio_classify(const LaunchArgs &a, uint8_t *cls, uint32_t *pos, uint32_t *list_near, uint32_t *list_far, WratioStatus *st);
hipError_t launch_take(const uint32_t *off, const uint8_t *val, const uint32_t *list, uint32_t m, uint32_t *out_off, uint8_t *out_val,
                       uint32_t *sums, hipStream_t stream);
hipError_t launch_wratio_combine(const LaunchArgs &a, const uint8_t *cls, const uint32_t *pos, const double *s_near, const double *s_far0,
                                 const double *s_far1);
hipError_t launch_max_f64(const double *x, const double *y, double *out, uint64_t n, hipStream_t stream);
// out[i] = the rule of partial_token_set_ratio over rec[i] and p[i] = partial_ratio(ab, ba)
hipError_t launch_partial_token_set_epilogue(const TokenSetRec *rec, const double *p, double *out, uint64_t n, hipStream_t stream);

// Nearest match by bounded edit distance (strsim_nearest_kernels.h), measure 0 (Levenshtein) or 6 (OSA).  The strings of both
// sides are packed by launch_match_pack first; launch_nearest_order then puts them in length order on the device (histograms,
// scan, scatter; the histograms must be zeroed), and launch_nearest_lane writes splits x nq x match_lane_k(k) partial lists in
// the encoding of k_match_merge (score -(double)d).  SweepLaneArgs is what the two length-ordered lane kernels take alike.
struct NearestOrderArgs {
    const uint32_t *qmeta; uint32_t nq;                // queries (k_match_pack)
    const uint32_t *cwords, *cmeta; uint32_t nc;       // candidates
    uint32_t *qhist, *chist;                           // NEAREST_BUCKETS words each, zeroed
    uint32_t *qstart, *cstart;                         // NEAREST_BUCKETS + 1 words each
    uint32_t *qcur, *ccur;                             // NEAREST_BUCKETS words each
    uint32_t *qperm;                                   // nq: the queries in length order, the slow ones last
    uint32_t *swords, *smeta, *sidx;                   // the fast candidates in length order: 8 words, meta, original index
    hipStream_t stream;
};
hipError_t launch_nearest_order(const NearestOrderArgs &a);
struct SweepLaneArgs {
    const uint32_t *qwords, *qmeta, *qperm, *qstart; uint32_t nq;
    const uint32_t *swords, *smeta, *sidx, *cstart;
    uint32_t splits, k;
    double *pscore; uint32_t *pidx;
    hipStream_t stream;
};
struct NearestLaneArgs {
    SweepLaneArgs s;
    uint32_t max_distance;
};
hipError_t launch_nearest_lane(int measure, const NearestLaneArgs &a);
// fallback distances -> scores -(double)d for launch_match_fold_cols / _rows; the merged scores -> distances (0xFFFFFFFF where the
// index is empty)
hipError_t launch_nearest_scores(const uint32_t *dist, uint64_t n, double *score, hipStream_t stream);
hipError_t launch_nearest_finish(const double *score, const uint32_t *index, uint64_t n, uint32_t *dist, hipStream_t stream);

// Top-k search by Indel similarity (strsim_extract_kernels.h).  Both sides packed by launch_match_pack and put in length order by
// launch_nearest_order; launch_extract_lane writes splits x nq x match_lane_k(k) partial lists in the encoding of k_match_merge.
// tab: the device copy of the rank table (strsim_extract.h); rlimit >= 1: the number of ranks the cutoff admits.
struct ExtractTable;
struct ExtractLaneArgs {
    SweepLaneArgs s;
    const ExtractTable *tab; uint32_t rlimit;
};
hipError_t launch_extract_lane(const ExtractLaneArgs &a);

// The full score matrix (strsim_cdist_kernels.h), measures 0 .. 4 and 8 (Indel).  Both sides packed by launch_match_pack;
// launch_cdist_lane writes out[i * ld + j] for every pair of split s's candidates [s * per, ...), 0.0 where a side is outside the
// lane class.  tab: the quotient table (measures 0 .. 2), the Indel score table of strsim_cdist.h (8), unused otherwise.
// launch_cdist_put_col: nb columns of nq pairwise scores into columns clist[b], the rows of slow queries left alone;
// launch_cdist_cutoff: the cutoff rule over rows qlist[b].
struct CdistLaneArgs {
    const uint32_t *qwords, *qmeta; uint32_t nq;
    const uint32_t *cwords, *cmeta; uint32_t nc;
    uint32_t splits, per;
    const double *tab;
    double cutoff;
    double *out; uint64_t ld;
    hipStream_t stream;
};
hipError_t launch_cdist_lane(int measure, const CdistLaneArgs &a);
hipError_t launch_cdist_put_col(const double *scores, const uint32_t *clist, uint32_t nb, const uint32_t *qmeta, uint32_t nq, double cutoff,
                                double *out, uint64_t ld, hipStream_t stream);
hipError_t launch_cdist_cutoff(double *out, const uint32_t *qlist, uint32_t nb, uint32_t nc, uint64_t ld, double cutoff, hipStream_t stream);

// Threshold join (strsim_join_kernels.h; the rules are in strsim_join.h).  Both sides packed by launch_match_pack and put in
// length order by launch_nearest_order, once per call.  JoinLaneArgs: what every join's lane sweep takes; what one sweep adds
// (here the rank table and rlimit >= 1) is its launcher's own argument.  launch_join_lane(false) stores the hits of (split, query
// i) at cnt[split * nq + i]; launch_join_indptr turns the `lists` counts of every query (the splits, then the fallback's list) into
// their prefix in place and the totals into indptr (nq + 1 words; sums: join_scan_blocks(nq) words); launch_join_lane(true) stores
// every hit inside the segment the counts gave it.  launch_join_slow: nb columns of pairwise scores of slow queries (side 0: nc
// scores each) or slow candidates (side 1: nq scores each) counted into / stored in the fallback's list fb (nq words; cur: nq
// cursors, zeroed before the fill).  launch_join_sort_rows: every row by candidate index.
struct JoinLaneArgs {
    const uint32_t *qwords, *qmeta, *qperm, *qstart; uint32_t nq;
    const uint32_t *swords, *smeta, *sidx, *cstart;
    uint32_t splits;
    uint32_t upper;
    uint32_t *cnt;
    uint32_t *map; uint64_t map_words; uint32_t map_shift; // the hit map: ceil(nq / 64) x map_words words
    const uint64_t *indptr;
    uint32_t *out_index; double *out_score;
    hipStream_t stream;
};
hipError_t launch_join_lane(bool fill, const JoinLaneArgs &a, const ExtractTable *tab, uint32_t rlimit);
hipError_t launch_join_indptr(uint32_t *cnt, uint32_t nq, uint32_t lists, uint64_t *indptr, uint64_t *sums, hipStream_t stream);
struct JoinSlowArgs {
    const double *scores; const uint32_t *list; uint32_t nb;
    const uint32_t *qmeta; uint32_t nq, nc;
    double cutoff; uint32_t upper;
    uint32_t *fb, *cur; const uint64_t *indptr;
    uint32_t *out_index; double *out_score;
    hipStream_t stream;
};
hipError_t launch_join_slow(int side, bool fill, const JoinSlowArgs &a);
hipError_t launch_join_sort_rows(const uint64_t *indptr, uint32_t nq, uint32_t nc, uint32_t *index, double *score, hipStream_t stream);

// Threshold join by a reference measure 0 .. 4 (strsim_match_join_kernels.h; the rule is in strsim_match_join.h): the sweep that
// stands where launch_join_lane stands, everything around it is the join's.  qtab: the quotient table (measures 0 .. 2), need: the
// lengths a query of each length visits, passed by value.
struct MatchJoinNeed;
hipError_t launch_match_join_lane(int measure, bool fill, const JoinLaneArgs &a, const double *qtab, const MatchJoinNeed &need, double min_score);

// Threshold join by q-gram similarity (strsim_qgram_join_kernels.h; the rule is in strsim_qgram_join.h): the sweep that stands where
// launch_join_lane stands.  kind: STRSIM_QGRAM_*, q: 1..3, set: the set mode.  Set mode reads `first`, one word per candidate in
// length order (nc words), which launch_qgram_join_first fills behind launch_nearest_order; multiset mode takes nullptr.
hipError_t launch_qgram_join_first(uint32_t q, const JoinLaneArgs &a, uint32_t nc, uint32_t *first);
hipError_t launch_qgram_join_lane(int kind, uint32_t q, bool set, bool fill, const JoinLaneArgs &a, const uint32_t *first, const MatchJoinNeed &need,
                                  double min_score);

// Join by integer edit distance (strsim_distance_join_kernels.h; the rules are in strsim_distance_join.h): the sweep that stands
// where launch_join_lane stands.  kind: EDIT_LEVENSHTEIN, EDIT_OSA or EDIT_DAMERAU; need: |lq - lc| <= max_distance.  The hits carry
// -(double)d in a.out_score; launch_distance_join_finish turns n of them into the uint32 distances.
hipError_t launch_distance_join_lane(int kind, bool fill, const JoinLaneArgs &a, const MatchJoinNeed &need, uint32_t max_distance);
hipError_t launch_distance_join_finish(const double *score, uint64_t n, uint32_t *dist, hipStream_t stream);

// Connected components of a CSR graph (strsim_components_kernels.h; the rules are in strsim_components.h).
// launch_components_identity: the labels of a graph without edges, one launch.  launch_components: init, link, compress, the join's
// three scan kernels over the root flags and the rank -- seven launches whatever the graph holds.  parent: rows words; scan: rows
// 64-bit words; sums: join_scan_blocks(rows) words; status: {count, indices out of range}.
hipError_t launch_components_identity(uint32_t rows, uint32_t *out_root, uint32_t *out_cluster, hipStream_t stream);
struct ComponentsArgs {
    const uint64_t *indptr; const uint32_t *index; uint32_t rows; uint64_t nnz;
    uint32_t *parent; uint64_t *scan, *sums, *status;
    uint32_t *out_root, *out_cluster;
    hipStream_t stream;
};
constexpr uint32_t COMPONENTS_LAUNCHES = 7u;
hipError_t launch_components(const ComponentsArgs &a);

} // namespace strsim

