/*
 * strsim_amd.h -- C ABI of the MI355X (gfx950) pairwise string-similarity library.
 *
 * This is the drop-in boundary for the hot path of foxcroftjn/polars-strsim: everything the
 * reference computes inside `strsim::parallel_apply` (reference src/expressions/strsim.rs:41-107) and
 * the five `SimilarityFunction::compute` bodies (:125-162, :180-245, :257-272, :286-308, :322-345).
 *
 * Two layers are exported from the same shared library (libpolars_strsim_amd.so):
 *
 *   1. the thin kernel ABI below (`strsim_*`): Arrow Utf8 offsets+values buffers in, f64 column out.
 *      This is what a Rust host (the reference's `parallel_apply`) would bind through `extern "C"`
 *      after flattening its `StringChunked` -- see INTEGRATION.md for the binding stub.
 *   2. the Polars plugin ABI (`_polars_plugin_*`, include/polars_plugin_abi.h): the symbols the
 *      reference's `#[polars_expr]` macro generates (reference src/expressions/mod.rs:8-31), so the
 *      library can be dropped into the `polars_strsim` package directory unchanged.
 *
 * Plain pointers and sizes only; no C++/torch types.  All functions return a strsim_status_t
 * (0 = OK) unless stated otherwise; on error a message is available from
 * strsim_last_error_message() (thread-local).  Nothing here ever computes on the CPU: without a
 * usable GPU every compute entry point fails with STRSIM_ERR_NO_DEVICE.
 */
#ifndef STRSIM_AMD_H
#define STRSIM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STRSIM_ABI_VERSION 0x00010007u /* major<<16 | minor; 1.1: strsim_pairs_device_small, strsim_codec_patch_indirect; 1.2: strsim_ctx_retire_oldest, strsim_offsets_from_lengths; 1.3: one-launch calls (strsim_ctx_set_stream_ordered, strsim_ctx_last_late_rows); 1.4: one-launch calls are OPT-IN -- a new context completes rows in stream order, as in 1.2; 1.5: strsim_column_from_views_bounded, strsim_codec_decode_gathered_from, strsim_gather_*, STRSIM_ERR_EARLIER_CALL; 1.6: strsim_gather_f64_ranges, strsim_gather_comm_count, strsim_ctx_get_stream_ordered; 1.7: strsim_best_match_device, strsim_best_match_host */

#if defined(__GNUC__)
#define STRSIM_API __attribute__((visibility("default")))
#else
#define STRSIM_API
#endif

/* Mirrors `enum SimilarityFunctionType` (reference strsim.rs:9-15). */
typedef enum strsim_measure {
    STRSIM_LEVENSHTEIN   = 0, /* normalised Levenshtein similarity, strsim.rs:125-162 */
    STRSIM_JARO          = 1, /* strsim.rs:180-245 */
    STRSIM_JARO_WINKLER  = 2, /* strsim.rs:257-272 */
    STRSIM_JACCARD       = 3, /* character-multiset Jaccard, strsim.rs:286-308 */
    STRSIM_SORENSEN_DICE = 4, /* character-multiset Sorensen-Dice, strsim.rs:322-345 */
    STRSIM_NUM_MEASURES  = 5, /* the reference's five; the value 5 itself is not a measure */
    STRSIM_OSA           = 6, /* optimal string alignment (restricted Damerau-Levenshtein: no substring is edited twice), normalised
                                 like STRSIM_LEVENSHTEIN: 1.0 when a == b or both are empty, else 1.0 - d / max(|a|, |b|) over Unicode
                                 scalar values.  Pairwise entry points only (strsim_pairs_device, _small, strsim_pairs_host);
                                 not a measure of the reference */
    STRSIM_INDEL         = 8, /* Indel (longest common subsequence) similarity, rapidfuzz's fuzz.ratio / 100: with l = LCS(a, b) and
                                 d = |a| + |b| - 2 l (insertions and deletions only, a substitution costs 2), 1.0 when |a| + |b| == 0,
                                 else 1.0 - d / (|a| + |b|) over Unicode scalar values (these two f64 operations, not 2 l / (|a| + |b|)).
                                 Pairwise entry points and strsim_distance_*; not a measure of the reference.  8, not 7: ids 5 and 7
                                 stay unassigned, callers were told (and tests hold) that every entry point refuses them */
    STRSIM_PARTIAL_RATIO = 10,/* partial ratio, rapidfuzz's fuzz.partial_ratio / 100: the best STRSIM_INDEL score of the shorter string
                                 (the needle, m scalar values) against a window of the longer one (n values) -- its proper prefixes
                                 of 1 .. m-1 values, every substring of m values, its proper suffixes of m-1 .. 1 values (n + m - 1
                                 windows; for n > m the whole longer string is NOT one of them, so the result can be below
                                 STRSIM_INDEL's).  Equal lengths: the larger of the two directions.  Both empty: 1.0; one empty: 0.0.
                                 It is the maximum at every needle length (rapidfuzz's heuristic for needles of more than 64
                                 characters is not followed).  Pairwise entry points and strsim_partial_alignment_*; 10, not 9: ids
                                 5, 7 and 9 stay unassigned and refused */
    STRSIM_TOKEN_SORT_RATIO = 14, /* rapidfuzz's fuzz.token_sort_ratio / 100: STRSIM_INDEL of join(sorted(tokens(a))) and
                                 join(sorted(tokens(b))), bit for bit.  Whitespace is Python's str.isspace set (29 code points: U+0009-000D,
                                 001C-001F, 0020, 0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000); tokens are the maximal runs
                                 of other scalar values (a NUL is a token character); token order is lexicographic by scalar value, a
                                 proper prefix first (= bytewise order of the UTF-8); join puts one U+0020 between tokens; duplicates
                                 are kept.  Two tokenless strings: 1.0; exactly one: 0.0.  Pairwise entry points only */
    STRSIM_TOKEN_SET_RATIO = 16,  /* rapidfuzz's fuzz.token_set_ratio / 100 over the SETS A, B of tokens (tokenised as above): 0.0 when A
                                 or B is empty; 1.0 when A & B is not empty and A - B or B - A is; else, with sect, ab, ba the joined
                                 sorted A & B, A - B, B - A of sl, la, lb scalar values, sep = (sl > 0), sab = sl + sep + la,
                                 sba = sl + sep + lb, d = indel_distance(ab, ba) and E(d, s) = 1.0 when s == 0 else 1.0 - d / s:
                                 r0 = E(d, sab + sba) when sl == 0, else max(r0, E(sep + la, sl + sab), E(sep + lb, sl + sba)) -- the
                                 maximum of STRSIM_INDEL over the pairs of sect, sect + " " + ab, sect + " " + ba.  Pairwise entry
                                 points only.  14 and 16: ids 5, 7, 9, 11 and 12 stay unassigned and refused */
    /* Compositions of the measures above (rapidfuzz's fuzz.* / 100, no processor), pairwise entry points only; the odd ids up to
       25 stay unassigned and refused.  Tokens, sorting, join, A, B, ab, ba as for ids 14 and 16. */
    STRSIM_TOKEN_RATIO = 18,      /* max(STRSIM_TOKEN_SORT_RATIO, STRSIM_TOKEN_SET_RATIO) */
    STRSIM_PARTIAL_TOKEN_SORT_RATIO = 20, /* STRSIM_PARTIAL_RATIO of join(sorted(tokens(a))) and join(sorted(tokens(b))) */
    STRSIM_PARTIAL_TOKEN_SET_RATIO = 22,  /* 0.0 when A or B is empty; 1.0 when A & B is not empty; else STRSIM_PARTIAL_RATIO of ab, ba */
    STRSIM_PARTIAL_TOKEN_RATIO = 24,      /* max(STRSIM_PARTIAL_TOKEN_SORT_RATIO, STRSIM_PARTIAL_TOKEN_SET_RATIO) */
    STRSIM_WRATIO = 26            /* rapidfuzz's fuzz.WRatio / 100.  With la, lb the scalar values of the RAW strings, lo = min, hi = max,
                                 r = STRSIM_INDEL(a, b): 0.0 when lo == 0; when 2 hi < 3 lo: max(r, STRSIM_TOKEN_RATIO * 0.95); else, with
                                 ps = 0.9 when hi <= 8 lo and 0.6 otherwise: max(r, STRSIM_PARTIAL_RATIO(a, b) * ps,
                                 (STRSIM_PARTIAL_TOKEN_RATIO * 0.95) * ps) -- f64 products in exactly this association.  The rows
                                 are classified on the device and each family runs over its own rows only
                                 (strsim_ctx_last_wratio_rows) */
} strsim_measure_t;

/* Entry points of strsim_measure_supported(). */
typedef enum strsim_entry_point {
    STRSIM_ENTRY_PAIRWISE   = 0, /* strsim_pairs_device, strsim_pairs_device_small, strsim_pairs_host */
    STRSIM_ENTRY_BEST_MATCH = 1, /* strsim_best_match_device, strsim_best_match_host */
    STRSIM_ENTRY_CODEC      = 2  /* strsim_codec_create */
} strsim_entry_point_t;

typedef enum strsim_status {
    STRSIM_OK              = 0,
    STRSIM_ERR_SHAPE       = 1, /* reference ShapeMismatch, strsim.rs:48-52 */
    STRSIM_ERR_ARG         = 2, /* null pointer / bad enum / bad size */
    STRSIM_ERR_NO_DEVICE   = 3, /* no usable HIP device: there is no CPU fallback */
    STRSIM_ERR_HIP         = 4, /* a HIP runtime call failed (message has the detail) */
    STRSIM_ERR_OOM         = 5,
    STRSIM_ERR_DTYPE       = 6, /* plugin ABI: input is not a string column (reference `.str()?`, strsim.rs:46-47) */
    STRSIM_ERR_INTERNAL    = 7,
    STRSIM_ERR_EARLIER_CALL = 8 /* strsim_pairs_device*: retiring EARLIER pending calls at a wrap of the context's ring of 32 failed
                                   (message has the detail); THIS call was not enqueued and none of its buffers was touched */
} strsim_status_t;

typedef struct strsim_ctx strsim_ctx_t; /* one device + one stream + its workspace; not thread-safe: one ctx per thread */

/* (major<<16)|minor of this ABI. */
STRSIM_API uint32_t strsim_abi_version(void);

/* NUL-terminated description of the last error raised on the calling thread ("" if none). */
STRSIM_API const char *strsim_last_error_message(void);

/* 1 if `entry_point` (strsim_entry_point_t) accepts `measure`, else 0 -- answered from the tables the argument checks of those
 * entry points use, without a device or a context.  The way to detect a measure: the ABI version does not move for one (STRSIM_OSA
 * came within 1.7), and the compute calls test for a NULL context before they look at the measure.  Unknown entry points: 0. */
STRSIM_API uint32_t strsim_measure_supported(int measure, int entry_point);

/* Number of usable HIP devices (0 when there is none; never fails). */
STRSIM_API int strsim_device_count(void);

/* Create a context on `device`.  `hip_stream` is a hipStream_t to enqueue on (e.g. the host
 * framework's current stream); NULL makes the context create and own a non-blocking stream. */
STRSIM_API int strsim_ctx_create(int device, void *hip_stream, strsim_ctx_t **out_ctx);
STRSIM_API void strsim_ctx_destroy(strsim_ctx_t *ctx);

/* The stream work is enqueued on (a hipStream_t). */
STRSIM_API void *strsim_ctx_stream(strsim_ctx_t *ctx);

/*
 * Enqueue one pass of `measure` over two DEVICE-RESIDENT Utf8 column shards.
 *
 * Column layout (Arrow "u", rebased): `offsets` = uint32[rows+1] with offsets[0] == 0... (any
 * monotone base is accepted), `values` = the packed UTF-8 bytes [0, offsets[rows]).  A side with
 * rows == 1 is the "Utf8 literal" of strsim.rs:48-52 and is broadcast against every row of the
 * other side (strsim.rs:61-66).  Otherwise a_rows must equal b_rows, else STRSIM_ERR_SHAPE.
 * `out` = double[out_rows] on the same device, out_rows = max(a_rows, b_rows).
 * Nulls are not seen here: like the reference's arity helpers the kernels compute on the bytes under
 * every slot; validity is combined by the caller (the plugin layer does it).
 *
 * STRSIM_OSA: rows where both strings are ASCII and at most 64 bytes are one pair per lane, every other row one pair per wave
 * (any length: patterns beyond 2048 scalar values use a scratch buffer the context grows).  All rows are complete in stream
 * order (strsim_ctx_last_long_rows / _last_late_rows report 0 for such a call), but the call waits once for the stream after
 * its first kernel (a read-back of how many rows need the second kernel and how long their patterns are), so everything
 * enqueued on the context's stream before it has completed when it returns.  Its kernels read only the bytes the offsets
 * describe.  strsim_ctx_set_stream_ordered(ctx, 0) does not change an OSA call.
 *
 * STRSIM_INDEL: the same protocol and the same reports as STRSIM_OSA, with other tiers: rows where both strings are ASCII and at
 * most 128 bytes are one pair per lane (strsim_ctx_last_wave_rows is 0 for a column of such rows), every other row one pair per
 * wave (any length).  A literal that is not ASCII or longer than 128 bytes sends every row to the second kernel.
 *
 * STRSIM_PARTIAL_RATIO: the same protocol and the same reports as STRSIM_OSA.  Rows where both strings are ASCII and at most 32
 * bytes are one pair per lane (strsim_ctx_last_wave_rows is 0 for a column of such rows), every other row one pair per wave (any
 * UTF-8, any length; tables beyond 16 KB use a scratch buffer the context grows; needles of more than 64 scalar values cost
 * O(n m ceil(m / 64)) word steps a pair).  Its kernels read only the bytes the offsets describe.
 *
 * STRSIM_TOKEN_SORT_RATIO, STRSIM_TOKEN_SET_RATIO: the columns are first rewritten on the device into scratch the context grows with
 * the call -- the sort form normalises each column (a literal stays one row), the set form writes the two difference columns at
 * full length (about one copy of each input column's bytes, 4 bytes of offsets and 4 of work list a row and side; the set form 20
 * more a row) -- and STRSIM_INDEL's two kernels then run over them; every row is complete in stream order.  Such a call waits
 * for the stream twice: once at its start for the columns' byte sizes and longest rows (they size the scratch; a failed
 * reservation is STRSIM_ERR_OOM), once as STRSIM_OSA does.  Rows whose strings are ASCII with at most 64 bytes and 16 tokens are
 * rewritten one string per lane, every other row one string per wave (any UTF-8, any length, any token count);
 * strsim_ctx_last_token_wave_rows() counts the latter.  A token_sort_ratio call reports strsim_ctx_last_wave_rows as STRSIM_INDEL
 * does; a token_set_ratio call is not a pending call of strsim_ctx_synchronize and leaves that counter alone.  The kernels read
 * only the bytes the offsets describe.
 *
 * Reads beyond the strings: the kernels copy the values of a block of rows in whole 16-byte chunks, from the
 * 16-byte-aligned address at or below the block's first byte (a_values + a_offsets[first row]) up to the chunk that
 * holds the column's last byte (a_values + a_offsets[a_rows]) -- up to 15 bytes in front of and behind the bytes the
 * offsets describe.  Those reads stay inside the 16-byte-aligned chunks the column itself touches (so inside its
 * pages); bytes in front belong to whatever precedes the column in the caller's buffer and only ever sit beside a
 * string in a staging area, bytes behind the column's last byte are replaced by zeros before any row looks at them.
 * Nothing outside [a_offsets[0], a_offsets[a_rows]) can change a result.
 *
 * The call is asynchronous: it returns once the kernels are enqueued on the context's stream.
 * Results are complete after strsim_ctx_synchronize() (or strsim_ctx_retire_oldest() of this call).
 * All buffers of a call must stay valid until then.
 *
 * What the stream alone guarantees: every row of strings <= STRSIM_WAVE_PATH_MAX_BYTES is complete in stream
 * order (work enqueued on strsim_ctx_stream() behind the call sees it); rows with a longer string are always
 * finished by a pass that strsim_ctx_synchronize() / strsim_ctx_retire_oldest() launches
 * (strsim_ctx_last_long_rows() tells).
 *
 * One-launch calls (opt-in since ABI 1.4: strsim_ctx_set_stream_ordered(ctx, 0)): a context whose last retired
 * call had every row finished by the one-pair-per-lane kernel (both strings <= STRSIM_LANE_PATH_MAX_BYTES, ASCII
 * -- the common column) enqueues the NEXT call as that kernel alone: ONE launch instead of five.  If such a call
 * does hold longer or non-ASCII rows, the kernels for them are launched when the call is retired, i.e. AFTER
 * anything the caller enqueued behind the call -- strsim_ctx_last_late_rows() tells, and the calls after it enqueue
 * all their kernels up front again.  For callers that retire every call (strsim_ctx_retire_oldest /
 * strsim_ctx_synchronize) before they consume its results, and look at strsim_ctx_last_late_rows() if they copied
 * results out early: the plugin layer does.  A pending one-launch call owns a "not finished yet" mask (20 bytes per 64 rows)
 * until it is retired, so a caller that keeps k calls in flight holds k of them.  The library never retires a call the
 * caller has not asked it to, except when more than 32 calls are in flight on one context: then everything pending is
 * retired inside strsim_pairs_device (a stream synchronise) and what that finished late is added to the next
 * retirement's strsim_ctx_last_late_rows().  If retiring them fails there, the error is THEIRS: the call returns
 * STRSIM_ERR_EARLIER_CALL and has not been enqueued (ABI 1.5; before, it returned the earlier call's own code).
 */
STRSIM_API int strsim_pairs_device(strsim_ctx_t *ctx, int measure,
                        const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                        const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                        double *out, uint64_t out_rows);

/* strsim_pairs_device for a SMALL call that the caller synchronises right away (strsim_pairs_host's in-place path, the
 * plugin's direct path; reference: one `compute` per row on the calling thread, strsim.rs:53-70).  May block until the
 * one-pair-per-lane kernel has finished: when that kernel leaves no row behind -- short ASCII strings, the common case --
 * the call is complete after one kernel launch and nothing is pending; otherwise the remaining kernels are enqueued and the
 * call completes in strsim_ctx_synchronize() like any other.  Same arguments and errors as strsim_pairs_device. */
STRSIM_API int strsim_pairs_device_small(strsim_ctx_t *ctx, int measure, const uint32_t *a_offsets, const uint8_t *a_values,
                                         uint64_t a_rows, const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                         double *out, uint64_t out_rows);

/*
 * All five measures of the same two column shards in one call (BASELINE config 4): the rows that fit the
 * lane-per-pair path are read once and produce five outputs from one set of bit-planes; `outs` is indexed by
 * strsim_measure_t, five device buffers of out_rows doubles.  Same asynchronous contract as above.
 */
STRSIM_API int strsim_pairs_device_all(strsim_ctx_t *ctx,
                            const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                            const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                            double *const outs[5], uint64_t out_rows);

/* Wait for everything enqueued through this context and surface any deferred error. */
STRSIM_API int strsim_ctx_synchronize(strsim_ctx_t *ctx);

/* 1 (default): every call enqueues all its kernels up front (results of rows <= STRSIM_WAVE_PATH_MAX_BYTES complete in stream
 * order); 0: calls that are expected to need the first kernel only are one launch (see strsim_pairs_device).  Takes effect
 * with the next call; calls already pending keep the mode they were enqueued in. */
STRSIM_API int strsim_ctx_set_stream_ordered(strsim_ctx_t *ctx, int enable);
/* The mode the NEXT call of the context is enqueued in: 1 = stream-ordered (the default), 0 = one-launch calls (ABI 1.6). */
STRSIM_API int strsim_ctx_get_stream_ordered(strsim_ctx_t *ctx);

/*
 * Same contract with HOST-RESIDENT buffers: stages the shards to the device, runs the kernels and
 * copies the f64 column back; synchronous.  Calls of up to 65 536 rows (and 2 MiB of values per
 * column) are gathered in one pinned block the context owns and computed there in place through the
 * device's mapping of host memory -- no copy engine, ~37 us per small call instead of ~70.
 */
STRSIM_API int strsim_pairs_host(strsim_ctx_t *ctx, int measure,
                      const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                      const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                      double *out, uint64_t out_rows);

/*
 * Best match (ABI 1.7): for every query row i, the k candidates j with the highest score(i, j), where score(i, j) is bit for bit
 * what strsim_pairs_device(measure, queries[i], candidates[j]) returns.  Row-major outputs of q_rows x k: out_index (uint32)
 * and out_score (double).  A query's slots are in descending order of the score; ties go to the lower candidate index.  A
 * candidate with score < min_score is never reported (-INFINITY or 0.0 reports every candidate).  Slots left empty (k > c_rows,
 * or too few candidates pass min_score) hold index 0xFFFFFFFF and score NaN.
 *
 * 1 <= k <= STRSIM_BEST_MATCH_MAX_K, q_rows <= 2^32 - 1, c_rows <= 2^32 - 2; c_rows == 0 is allowed (every slot empty) and
 * q_rows == 0 is a no-op.  A NaN min_score, a NULL buffer of a non-empty side or output, a bad measure or k: STRSIM_ERR_ARG.
 * The arguments are checked first, the context last (a NULL ctx is STRSIM_ERR_ARG too): no argument error needs a device.
 * Nulls are not seen here (as in strsim_pairs_device): a caller drops null candidates and maps the indices back.
 *
 * Device-resident: the same column layout as strsim_pairs_device.  Reads beyond the strings: none by the kernels of this call
 * (each string is read byte by byte within its offsets); pairs with a string longer than STRSIM_LANE_PATH_MAX_BYTES or a
 * non-ASCII one go through strsim_pairs_device (one side as the literal) and read what it documents.
 * The call waits once for the stream (a read-back of how many strings fall outside the one-pair-per-lane class).  Without such
 * strings it then returns with the search enqueued: results are complete after strsim_ctx_synchronize(), or in stream order.
 * With them it runs those pairs through strsim_pairs_device batch by batch and synchronises the context (strsim_ctx_synchronize)
 * after each batch, so everything enqueued on the context before the call is complete when it returns.
 */
#define STRSIM_BEST_MATCH_MAX_K 16u
STRSIM_API int strsim_best_match_device(strsim_ctx_t *ctx, int measure,
                                        const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                        const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                        uint32_t k, double min_score, uint32_t *out_index, double *out_score);

/* The same with HOST-RESIDENT buffers (the column layout of strsim_pairs_host); synchronous. */
STRSIM_API int strsim_best_match_host(strsim_ctx_t *ctx, int measure,
                                      const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                      const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                      uint32_t k, double min_score, uint32_t *out_index, double *out_score);

/*
 * Bounded edit distances as integers (found by dlsym, like strsim_measure_supported: the ABI version stays 1.7).  `measure` is
 * STRSIM_LEVENSHTEIN (0: insert, delete, substitute), STRSIM_OSA (6: plus the restricted swap of two adjacent characters) or
 * STRSIM_INDEL (8: insert and delete only, d = |a| + |b| - 2 LCS(a, b); its similarity is 1.0 - d / (|a| + |b|), and the lane tier
 * takes ASCII rows of up to 128 bytes; a pair whose lengths differ by more than max_distance is decided without the DP); any
 * other id is STRSIM_ERR_ARG (strsim_measure_supported does not describe these two entry points).  d is over Unicode scalar values.
 * out[i] = d when d <= max_distance, else max_distance + 1 (rapidfuzz's score_cutoff convention); STRSIM_DISTANCE_UNBOUNDED is
 * no cutoff and max_distance = 0 an equality test.  With no cutoff, 1.0 - d / max(|a|, |b|) (1.0 when both are empty) is bit for
 * bit what strsim_pairs_device returns for the same measure.
 *
 * Shape rule, literal broadcast and out_rows as strsim_pairs_device; zero rows is a no-op.  The arguments are checked first and
 * the context last (a NULL ctx is STRSIM_ERR_ARG too): no argument error needs a device.  Rows where both strings are ASCII and
 * at most 64 bytes are one pair per lane, every other row one pair per wave (any length; patterns beyond 2048 scalar values use
 * a scratch buffer the context grows).  Every row is complete in stream order; the call waits once for the stream after its
 * first kernel (to size the second), so everything enqueued before it has completed when it returns.  It is not a pending call
 * of strsim_ctx_synchronize and adds nothing to strsim_ctx_last_long_rows / _last_late_rows.  Its kernels read only the bytes
 * the offsets describe.  The host variant stages the columns (strsim_pairs_host's copy path) and is synchronous.
 */
#define STRSIM_DISTANCE_UNBOUNDED 0xFFFFFFFFu
STRSIM_API int strsim_distance_device(strsim_ctx_t *ctx, int measure,
                                      const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                      const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                      uint32_t max_distance, uint32_t *out, uint64_t out_rows);
STRSIM_API int strsim_distance_host(strsim_ctx_t *ctx, int measure,
                                    const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                    const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                    uint32_t max_distance, uint32_t *out, uint64_t out_rows);

/*
 * q-gram similarity (found by dlsym, like the distance calls: the ABI version stays 1.7, and no measure id is added).  Strings are
 * sequences of Unicode scalar values; for q = 1, 2 or 3, G(s) is the multiset of the max(|s| - q + 1, 0) contiguous q-tuples of s.
 * Multiset mode (flags = 0): na = |G(a)|, nb = |G(b)|, I = the sum over the grams of min(count in a, count in b).  Set mode
 * (STRSIM_QGRAM_SET): na and nb are the numbers of distinct grams, I the number of grams present in both.  In this order:
 * a == b bytewise (both empty included) is 1.0; na == 0 or nb == 0 is 0.0; otherwise, by `kind`,
 *   STRSIM_QGRAM_JACCARD        I / (na + nb - I)
 *   STRSIM_QGRAM_SORENSEN_DICE  (2.0 * I) / (na + nb)
 *   STRSIM_QGRAM_OVERLAP        I / min(na, nb)
 *   STRSIM_QGRAM_COSINE         I / sqrt(na * nb), the product formed in 64-bit integers
 * each with correctly rounded f64 operations.  A NUL byte is a character like any other, and no gram holds padding.  At q = 1 in
 * multiset mode the first two are STRSIM_JACCARD and STRSIM_SORENSEN_DICE of strsim_pairs_device, bit for bit.
 *
 * Shape rule, literal broadcast and out_rows as strsim_pairs_device; zero rows is a no-op.  A kind outside 0..3, q outside 1..3 or
 * a flag bit other than STRSIM_QGRAM_SET is STRSIM_ERR_ARG; the arguments are checked first and the context last (a NULL ctx is
 * STRSIM_ERR_ARG too): no argument error needs a device.  Rows where both strings are ASCII and at most 64 bytes are one pair per
 * lane, every other row one pair per wave (any length; pairs of more than 2048 grams use a scratch buffer the context grows), and
 * strsim_ctx_last_wave_rows counts the latter when the call returns.  Every row is complete in stream order; the call waits once
 * for the stream after its first kernel (to size the second), so everything enqueued before it has completed when it returns.  It
 * is not a pending call of strsim_ctx_synchronize and adds nothing to strsim_ctx_last_long_rows / _last_late_rows.  Its kernels
 * read only the bytes the offsets describe.  The host variant stages the columns (strsim_pairs_host's copy path) and is synchronous.
 */
enum { STRSIM_QGRAM_JACCARD = 0, STRSIM_QGRAM_SORENSEN_DICE = 1, STRSIM_QGRAM_OVERLAP = 2, STRSIM_QGRAM_COSINE = 3 };
#define STRSIM_QGRAM_SET 1u /* flags bit 0: sets of grams instead of multisets; every other bit must be 0 */
STRSIM_API int strsim_qgram_device(strsim_ctx_t *ctx, int kind, uint32_t q, uint32_t flags,
                                   const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                   const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                   double *out, uint64_t out_rows);
STRSIM_API int strsim_qgram_host(strsim_ctx_t *ctx, int kind, uint32_t q, uint32_t flags,
                                 const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                 const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                 double *out, uint64_t out_rows);

/*
 * Unrestricted Damerau-Levenshtein similarity and distance (found by dlsym, like the distance calls: the ABI version stays 1.7, and
 * no measure id is added).  Strings are sequences of Unicode scalar values.  d(a, b) is the smallest number of insertions,
 * deletions, substitutions and swaps of two adjacent characters that turns a into b, where a substring may be edited any number of
 * times (Lowrance and Wagner 1975): ("ca", "abc") is 2, where STRSIM_OSA's restricted distance is 3.  Unlike that one, d is a metric;
 * levenshtein >= osa >= d >= | |a| - |b| | for every pair.  A NUL byte is a character like any other.
 *   strsim_damerau_*           1.0 when a == b bytewise or both are empty, else 1.0 - d / max(|a|, |b|) (STRSIM_OSA's two f64
 *                              operations; strsim::normalized_damerau_levenshtein)
 *   strsim_damerau_distance_*  d when d <= max_distance, else max_distance + 1; STRSIM_DISTANCE_UNBOUNDED: no cutoff, 0: an equality
 *                              test (strsim_distance_device's convention)
 * Shape rule, literal broadcast and out_rows as strsim_pairs_device; zero rows is a no-op.  The arguments are checked first and the
 * context last (a NULL ctx is STRSIM_ERR_ARG too): no argument error needs a device.  Rows where both strings are ASCII and at most
 * 32 bytes are one pair per lane, every other row one pair per wave (any length; pairs whose shorter string has more than 2048
 * bytes use a scratch buffer the context grows), and strsim_ctx_last_wave_rows counts the latter when the call returns.  The cost is
 * that of a cell DP, |a| |b| cells a pair: there is no bit-parallel form of this distance.  Every row is complete in stream order;
 * the call waits once for the stream after its first kernel (to size the second), so everything enqueued before it has completed
 * when it returns.  It is not a pending call of strsim_ctx_synchronize and adds nothing to strsim_ctx_last_long_rows /
 * _last_late_rows.  Its kernels read only the bytes the offsets describe.  The host variants stage the columns (strsim_pairs_host's
 * copy path) and are synchronous.
 */
STRSIM_API int strsim_damerau_device(strsim_ctx_t *ctx,
                                     const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                     const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                     double *out, uint64_t out_rows);
STRSIM_API int strsim_damerau_host(strsim_ctx_t *ctx,
                                   const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                   const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                   double *out, uint64_t out_rows);
STRSIM_API int strsim_damerau_distance_device(strsim_ctx_t *ctx,
                                              const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                              const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                              uint32_t max_distance, uint32_t *out, uint64_t out_rows);
STRSIM_API int strsim_damerau_distance_host(strsim_ctx_t *ctx,
                                            const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                            const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                            uint32_t max_distance, uint32_t *out, uint64_t out_rows);

/*
 * Hamming, prefix, postfix and LCSseq similarity, distance and count (found by dlsym, like the distance calls: the ABI version stays
 * 1.7, and no measure id is added).  Strings are sequences of Unicode scalar values; a NUL byte is a character like any other.  Each
 * kind is a count c(a, b) of what the two strings share, at most min(|a|, |b|):
 *   STRSIM_COMMON_HAMMING  positions i < min(|a|, |b|) with a_i == b_i
 *   STRSIM_COMMON_PREFIX   length of the longest common prefix
 *   STRSIM_COMMON_POSTFIX  length of the longest common suffix
 *   STRSIM_COMMON_LCSSEQ   length of the longest common subsequence
 * and the three calls derive their output from it as rapidfuzz.distance.{Hamming, Prefix, Postfix, LCSseq} do:
 *   strsim_common_count_*     c (the similarity of rapidfuzz)
 *   strsim_common_distance_*  d = max(|a|, |b|) - c (Hamming: mismatches plus the difference of the lengths, rapidfuzz's pad=True)
 *                             when d <= max_distance, else max_distance + 1; STRSIM_DISTANCE_UNBOUNDED: no cutoff, 0: an equality
 *                             test (strsim_distance_device's convention)
 *   strsim_common_*           1.0 - d / max(|a|, |b|), and 1.0 when both are empty (STRSIM_OSA's two f64 operations)
 * An unknown kind is STRSIM_ERR_ARG.  Shape rule, literal broadcast and out_rows as strsim_pairs_device; zero rows is a no-op.  The
 * arguments are checked first and the context last (a NULL ctx is STRSIM_ERR_ARG too): no argument error needs a device.  For the
 * three positional kinds, rows where both strings are ASCII and at most 32 bytes are one pair per lane, every other row one pair per
 * wave (any length, streamed: no scratch); STRSIM_COMMON_LCSSEQ has STRSIM_INDEL's tiers (ASCII and at most 128 bytes per lane).
 * strsim_ctx_last_wave_rows counts the rows of the wave tier when the call returns.  Every row is complete in stream order; the call
 * waits once for the stream after its first kernel (to size the second), so everything enqueued before it has completed when it
 * returns.  It is not a pending call of strsim_ctx_synchronize and adds nothing to strsim_ctx_last_long_rows / _last_late_rows.  Its
 * kernels read only the bytes the offsets describe.  The host variants stage the columns (strsim_pairs_host's copy path) and are
 * synchronous.
 */
enum { STRSIM_COMMON_HAMMING = 0, STRSIM_COMMON_PREFIX = 1, STRSIM_COMMON_POSTFIX = 2, STRSIM_COMMON_LCSSEQ = 3 };
STRSIM_API int strsim_common_device(strsim_ctx_t *ctx, int kind,
                                    const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                    const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                    double *out, uint64_t out_rows);
STRSIM_API int strsim_common_host(strsim_ctx_t *ctx, int kind,
                                  const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                  const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                  double *out, uint64_t out_rows);
STRSIM_API int strsim_common_distance_device(strsim_ctx_t *ctx, int kind,
                                             const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                             const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                             uint32_t max_distance, uint32_t *out, uint64_t out_rows);
STRSIM_API int strsim_common_distance_host(strsim_ctx_t *ctx, int kind,
                                           const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                           const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                           uint32_t max_distance, uint32_t *out, uint64_t out_rows);
STRSIM_API int strsim_common_count_device(strsim_ctx_t *ctx, int kind,
                                          const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                          const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                          uint32_t *out, uint64_t out_rows);
STRSIM_API int strsim_common_count_host(strsim_ctx_t *ctx, int kind,
                                        const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                        const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                        uint32_t *out, uint64_t out_rows);

/*
 * Partial ratio with its alignment (found by dlsym, like the distance calls: the ABI version stays 1.7).  out_score[i] is bit for
 * bit what strsim_pairs_device(STRSIM_PARTIAL_RATIO) returns for row i.  out_span is out_rows x 4 uint32, row-major: a_start, a_end,
 * b_start, b_end -- half open, in Unicode scalar values (not bytes).  The needle (the shorter string; a when the lengths are equal,
 * unless b as the needle scores strictly higher) spans (0, its length); the other string's span is the winning window.  Among
 * windows with the same score the one with the smallest end wins, then the smallest start, whatever the order a kernel visits
 * them in.  Both strings empty, or exactly one: all four are 0.
 *
 * Shape rule, literal broadcast and out_rows as strsim_pairs_device; zero rows is a no-op.  The arguments are checked first and
 * the context last (a NULL ctx is STRSIM_ERR_ARG too): no argument error needs a device.  The tiers are those of
 * STRSIM_PARTIAL_RATIO (ASCII rows of up to 32 bytes one pair per lane, every other row one pair per wave).  Every row is complete
 * in stream order; the call waits once for the stream after its first kernel (to size the second), so everything enqueued before
 * it has completed when it returns.  It is not a pending call of strsim_ctx_synchronize and adds nothing to
 * strsim_ctx_last_long_rows / _last_late_rows.  Its kernels read only the bytes the offsets describe.  The host variant stages
 * the columns (strsim_pairs_host's copy path) and is synchronous.
 */
STRSIM_API int strsim_partial_alignment_device(strsim_ctx_t *ctx,
                                               const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                               const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                               double *out_score, uint32_t *out_span, uint64_t out_rows);
STRSIM_API int strsim_partial_alignment_host(strsim_ctx_t *ctx,
                                             const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                             const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                             double *out_score, uint32_t *out_span, uint64_t out_rows);

/*
 * The token_sort transform itself (found by dlsym: the ABI version stays 1.7): row i of the output column is
 * join(sorted(tokens(row i))) as STRSIM_TOKEN_SORT_RATIO defines it, so that
 * strsim_pairs_device(STRSIM_INDEL) over two transformed columns is strsim_pairs_device(STRSIM_TOKEN_SORT_RATIO) over the
 * originals, bit for bit -- normalise once, compare many times; strsim_best_match_* and strsim_nearest_* over transformed columns
 * search without regard to token order.  out_offsets holds rows + 1 words and starts at 0; out_values holds out_capacity bytes.
 * A normalised string is never longer than its input, so the column's byte size (offsets[rows] - offsets[0]) always suffices;
 * a smaller capacity is STRSIM_ERR_ARG (the device variant learns the size from the device: it waits once for the stream at its
 * start, and makes no other wait).  The output is complete in stream order.  Zero rows: out_offsets[0] = 0.  The arguments are
 * checked first and the context last.  The host variant stages the column and is synchronous.
 * strsim_ctx_last_token_wave_rows: the rows the last token call of the context (these two, or a pairwise call of measure 14 or 16)
 * rewrote one string per wave, both columns added up; valid once the stream has completed that call.
 */
STRSIM_API int strsim_token_sort_device(strsim_ctx_t *ctx, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                                        uint32_t *out_offsets, uint8_t *out_values, uint64_t out_capacity);
STRSIM_API int strsim_token_sort_host(strsim_ctx_t *ctx, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                                      uint32_t *out_offsets, uint8_t *out_values, uint64_t out_capacity);
STRSIM_API uint64_t strsim_ctx_last_token_wave_rows(strsim_ctx_t *ctx);

/*
 * default_process and processed scoring (found by dlsym: the ABI version stays 1.7, strsim_measure_supported does not describe
 * them and no measure id is added).  default_process is rapidfuzz's utils.default_process made context-free: every scalar value c
 * of a row is mapped by m -- m(c) = U+0020 when c is neither alphanumeric (Python's str.isalnum) nor "_", else the first scalar
 * value of Python's c.lower() -- and U+0020 is then removed from both ends of the row; inner runs of spaces stay ("Apple, Inc."
 * becomes "apple  inc").  It equals re.sub(r"(?ui)\W", " ", s).strip().lower() except in two places: U+03A3 maps to U+03C3 in
 * every position (no final sigma), and U+0130 maps to "i" (its simple lower-case mapping, no U+0307 behind it).  m comes from a
 * table generated from Python (strsim_default_process_unicode_version names its Unicode version); strsim_default_process_char
 * returns m(cp) -- U+0020 for surrogates and values above U+10FFFF -- and, like the version call, needs no device.
 *
 * strsim_default_process_*: row i of the output column is default_process(row i); the same column layout, and any monotone offset
 * base, as strsim_token_sort_*.  out_offsets holds rows + 1 words and starts at 0; out_values holds out_capacity bytes.  A
 * processed row can be LONGER than its input (U+023A and U+023E grow from two bytes of UTF-8 to three):
 * STRSIM_DEFAULT_PROCESS_CAPACITY(bytes) = bytes + bytes / 2 always suffices, the exact size is out_offsets[rows].  The device
 * variant enqueues the measuring pass and the offset scan, waits once for the stream (the exact size, the column's bounds) and
 * enqueues the writing pass: the output is complete in stream order.  A capacity below the exact size is STRSIM_ERR_ARG and
 * nothing is written to out_values (out_offsets has been written); so is a column of more than (2^32 - 1) * 2 / 3 bytes, whose
 * processed form might not fit 32-bit offsets.  Zero rows: out_offsets[0] = 0.  The arguments are checked first and the context
 * last.  The host variant stages the column and is synchronous.  Rows of at most 64 ASCII bytes are rewritten one string per
 * lane, every other row one string per wave (any UTF-8, any length); strsim_ctx_last_process_wave_rows counts the latter for the
 * last call of the context (both sides of a processed-scoring call added up), valid when that call has returned.  The kernels
 * read only the bytes the offsets describe and write only a row's own output bytes; on malformed UTF-8 the result is unspecified
 * within those limits (a lead byte without all the continuation bytes it calls for counts as one space, so bytes + bytes / 2
 * suffices for any bytes at all).  Scratch: 4 bytes of work list a row and 36 KB for the table.
 *
 * strsim_pairs_processed_*: `measure` over the processed columns -- bit for bit strsim_pairs_device(measure) over
 * strsim_default_process_device of each side.  processor is STRSIM_PROCESS_DEFAULT; anything else is STRSIM_ERR_ARG, as is a
 * measure the pairwise entry point refuses.  Both sides are processed into scratch of the context that no flow of the pairwise
 * call uses (a literal stays a one-row literal): 4 bytes of offsets and 4 of work list a row and side, and the exact processed
 * bytes of each side (+ 64); a failed reservation is STRSIM_ERR_OOM.  That scratch holds the input columns of the pairwise call,
 * which a pending call's retirement reads again; so the call first retires every call of the context that is still pending, as the
 * wrap of the ring does (a wait for the stream and their long-string or deferred passes; what they finished late is reported with
 * the next strsim_ctx_synchronize / _retire_oldest; a failure there is STRSIM_ERR_EARLIER_CALL and this call is not enqueued) --
 * calls can be enqueued back to back.  The call waits once for the stream for both sides' sizes,
 * then runs strsim_pairs_device: what that documents for `measure` (further waits, strsim_ctx_synchronize, the counters) holds
 * from there on.  The host variant stages both columns and is synchronous.
 */
#define STRSIM_PROCESS_DEFAULT 1
#define STRSIM_DEFAULT_PROCESS_CAPACITY(bytes) ((uint64_t)(bytes) + (uint64_t)(bytes) / 2u)
STRSIM_API uint32_t strsim_default_process_char(uint32_t cp);
STRSIM_API const char *strsim_default_process_unicode_version(void);
STRSIM_API int strsim_default_process_device(strsim_ctx_t *ctx, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                                             uint32_t *out_offsets, uint8_t *out_values, uint64_t out_capacity);
STRSIM_API int strsim_default_process_host(strsim_ctx_t *ctx, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                                           uint32_t *out_offsets, uint8_t *out_values, uint64_t out_capacity);
STRSIM_API int strsim_pairs_processed_device(strsim_ctx_t *ctx, int measure, int processor,
                                             const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                             const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                             double *out, uint64_t out_rows);
STRSIM_API int strsim_pairs_processed_host(strsim_ctx_t *ctx, int measure, int processor,
                                           const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows,
                                           const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows,
                                           double *out, uint64_t out_rows);
STRSIM_API uint64_t strsim_ctx_last_process_wave_rows(strsim_ctx_t *ctx);

/*
 * STRSIM_TOKEN_RATIO .. STRSIM_WRATIO (ids 18 .. 26; strsim_measure_supported(id, STRSIM_ENTRY_PAIRWISE) detects them, the ABI
 * version stays 1.7).  Ids 18 .. 24 run the token transforms and the Indel / partial-ratio kernels over the whole frame.
 * STRSIM_WRATIO computes STRSIM_INDEL over every row into `out`, classifies the rows on the device and gathers the near rows and
 * the far rows into two sub-frames in context scratch (a literal side stays a literal); STRSIM_TOKEN_RATIO runs over the near
 * sub-frame, STRSIM_PARTIAL_RATIO and STRSIM_PARTIAL_TOKEN_RATIO over the far one, and a last kernel writes the rule's result.  A
 * sub-frame without rows launches nothing.  Scratch beyond the token calls': 5 bytes a row of classes and positions, 8 of lists, one
 * copy of each gathered column and 8 bytes a sub-score; a failed reservation is STRSIM_ERR_OOM.  None of
 * these calls is a pending call of strsim_ctx_synchronize; every row is complete in stream order.
 *
 * strsim_ctx_last_wratio_rows: how the last completed STRSIM_WRATIO call of the context routed its rows (found by dlsym).  Rows in
 * neither count had an empty string.  STRSIM_ERR_ARG when ctx is NULL (both counts are set to 0 when given).
 */
STRSIM_API int strsim_ctx_last_wratio_rows(strsim_ctx_t *ctx, uint64_t *near_rows, uint64_t *far_rows);

/*
 * Nearest match by bounded edit distance (found by dlsym, like the distance calls: the ABI version stays 1.7, and
 * strsim_measure_supported does not describe these two entry points).  `measure` is STRSIM_LEVENSHTEIN or STRSIM_OSA; any other
 * id is STRSIM_ERR_ARG.  d(i, j) is exactly what strsim_distance_device(measure, queries[i], candidates[j],
 * STRSIM_DISTANCE_UNBOUNDED) returns: the edit distance over Unicode scalar values.  Row-major outputs of q_rows x k (uint32):
 * query i gets the (up to) k candidates j with the smallest d(i, j) <= max_distance, in ascending order of d, ties to the lower
 * candidate index -- one total order, so the result does not depend on the order in which candidates are visited.  Slots left
 * empty hold index 0xFFFFFFFF and distance 0xFFFFFFFF.  STRSIM_DISTANCE_UNBOUNDED is no cutoff; max_distance = 0 reports exact
 * matches only.
 *
 * 1 <= k <= STRSIM_NEAREST_MAX_K, q_rows <= 2^32 - 1, c_rows <= 2^32 - 2; c_rows == 0 is allowed (every slot empty) and
 * q_rows == 0 is a no-op.  A NULL buffer of a non-empty side or output, a bad measure or k: STRSIM_ERR_ARG.  The arguments are
 * checked first, the context last (a NULL ctx is STRSIM_ERR_ARG too): no argument error needs a device.  Nulls are not seen here:
 * a caller drops null candidates and maps the indices back.
 *
 * Device-resident: the same column layout as strsim_pairs_device.  Reads beyond the strings: none by the kernels of this call
 * (each string is read byte by byte within its offsets).  Strings of at most 32 ASCII bytes are searched one query per lane, in
 * length order, visiting only candidate lengths that can still enter a list; every pair with a longer or non-ASCII side goes
 * through strsim_distance_device (that string as the literal, max_distance passed on) and reads what it documents.
 * The call waits once for the stream (a read-back of how many strings fall outside the one-query-per-lane class).  Without such
 * strings it then returns with the search enqueued: results are complete after strsim_ctx_synchronize(), or in stream order.
 * With them it runs those pairs through strsim_distance_device batch by batch, each of which waits for the stream.
 */
#define STRSIM_NEAREST_MAX_K 16u
STRSIM_API int strsim_nearest_device(strsim_ctx_t *ctx, int measure,
                                     const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                     const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                     uint32_t k, uint32_t max_distance, uint32_t *out_index, uint32_t *out_distance);

/* The same with HOST-RESIDENT buffers (the column layout of strsim_pairs_host); synchronous. */
STRSIM_API int strsim_nearest_host(strsim_ctx_t *ctx, int measure,
                                   const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                   const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                   uint32_t k, uint32_t max_distance, uint32_t *out_index, uint32_t *out_distance);

/*
 * Extract: top-k search by ratio or token_sort_ratio with a score cutoff -- rapidfuzz's process.extract / extractOne with
 * fuzz.ratio / 100 or fuzz.token_sort_ratio / 100 as the scorer (found by dlsym, like the distance and nearest calls: the ABI
 * version stays 1.7, and strsim_measure_supported does not describe these two entry points).  `scorer` is STRSIM_INDEL (8) or
 * STRSIM_TOKEN_SORT_RATIO (14); any other id is STRSIM_ERR_ARG.  score(i, j) is bit for bit what
 * strsim_pairs_device(scorer, queries[i], candidates[j]) returns; for scorer 14 that is indel(token_sort(q), token_sort(c)).
 * Row-major outputs of q_rows x k (uint32 index, f64 score): query i gets the (up to) k candidates j with the highest
 * score(i, j) >= score_cutoff, in descending order of score, ties to the lower candidate index -- one total order, so the result
 * does not depend on the order in which candidates are visited.  Slots left empty hold index 0xFFFFFFFF and a NaN score, as best
 * match's.  score_cutoff = -INFINITY or 0.0 reports everything, a cutoff above 1.0 nothing; NaN is STRSIM_ERR_ARG.
 *
 * 1 <= k <= STRSIM_EXTRACT_MAX_K, q_rows <= 2^32 - 1, c_rows <= 2^32 - 2; c_rows == 0 is allowed (every slot empty) and
 * q_rows == 0 is a no-op.  A NULL buffer of a non-empty side or output, a bad scorer or k: STRSIM_ERR_ARG.  The arguments are
 * checked first, the context last (a NULL ctx is STRSIM_ERR_ARG too): no argument error needs a device.  Nulls are not seen here:
 * a caller drops null candidates and maps the indices back.
 *
 * Device-resident: the same column layout as strsim_pairs_device.  Strings of at most 32 ASCII bytes are searched one query per
 * lane, in length order, visiting only candidate lengths whose best possible score 1 - ||q| - |c|| / (|q| + |c|) can still reach
 * the cutoff or enter a full list; every pair with a longer or non-ASCII side goes through strsim_pairs_device(STRSIM_INDEL)
 * (that string as the literal) and reads what it documents.  Scorer 14 first normalises both columns on the device with the
 * token_sort transform into scratch of the context (no string goes to the host) and then searches those; it updates
 * strsim_ctx_last_token_wave_rows like any token call.
 * Waits for the stream: scorer 14 waits once for the bounds of its columns; every call waits once for a read-back of how many
 * strings fall outside the one-query-per-lane class.  Without such strings it then returns with the search enqueued: results are
 * complete after strsim_ctx_synchronize(), or in stream order.  With them it runs those pairs through strsim_pairs_device batch
 * by batch, each of which waits for the stream.
 */
#define STRSIM_EXTRACT_MAX_K 16u
STRSIM_API int strsim_extract_device(strsim_ctx_t *ctx, int scorer,
                                     const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                     const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                     uint32_t k, double score_cutoff, uint32_t *out_index, double *out_score);

/* The same with HOST-RESIDENT buffers (the column layout of strsim_pairs_host); synchronous. */
STRSIM_API int strsim_extract_host(strsim_ctx_t *ctx, int scorer,
                                   const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                   const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                   uint32_t k, double score_cutoff, uint32_t *out_index, double *out_score);

/*
 * cdist: the full score matrix of queries x candidates -- rapidfuzz's process.cdist with scores / 100 (found by dlsym, like the
 * search calls: the ABI version stays 1.7, and strsim_measure_supported does not describe these two entry points).  `measure` is
 * one of the reference measures (ids 0 .. 4), STRSIM_INDEL (8) or STRSIM_TOKEN_SORT_RATIO (14); any other id is STRSIM_ERR_ARG.
 * out is row-major f64 with leading dimension out_ld >= c_rows: out[i * out_ld + j] is bit for bit what
 * strsim_pairs_device(measure, queries[i], candidates[j]) returns, except that a score < score_cutoff is stored as 0.0
 * (rapidfuzz's rule; score_cutoff = -INFINITY or 0.0 changes nothing, a cutoff above 1.0 gives all zeros, NaN is STRSIM_ERR_ARG).
 * Columns c_rows .. out_ld - 1 of every row are never written.
 *
 * q_rows <= 2^32 - 1, c_rows <= 2^32 - 2; q_rows == 0 or c_rows == 0 is a no-op.  out_ld < c_rows, a NULL buffer of a non-empty
 * side or a NULL out of a non-empty matrix, a bad measure or a NaN cutoff: STRSIM_ERR_ARG.  The arguments are checked first, the
 * context last (a NULL ctx is STRSIM_ERR_ARG too): no argument error needs a device.  Nulls are not seen here.
 *
 * Device-resident: the same column layout as strsim_pairs_device; out needs 8-byte alignment only.  Strings of at most 32 ASCII
 * bytes are scored one query per lane against every candidate and the scores leave through a tile of LDS in whole rows; every
 * pair with a longer or non-ASCII side goes through strsim_pairs_device (that string as the literal): a slow query straight into
 * its row, a slow candidate into one scratch column of q_rows doubles that is then scattered into its column.  Measure 14 first
 * normalises both columns on the device with the token_sort transform, as strsim_extract_device does.
 * Waits for the stream: measure 14 waits once for the bounds of its columns; every call waits once for a read-back of how many
 * strings fall outside the one-query-per-lane class.  Without such strings it then returns with the sweep enqueued: the matrix is
 * complete after strsim_ctx_synchronize(), or in stream order.  With them it runs those pairs through strsim_pairs_device batch by
 * batch, each of which waits for the stream.  Scratch the context cannot reserve is STRSIM_ERR_OOM.
 */
STRSIM_API int strsim_cdist_device(strsim_ctx_t *ctx, int measure,
                                   const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                   const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                   double score_cutoff, double *out, uint64_t out_ld);

/* The same with HOST-RESIDENT buffers (the column layout of strsim_pairs_host, out included); synchronous. */
STRSIM_API int strsim_cdist_host(strsim_ctx_t *ctx, int measure,
                                 const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                 const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                 double score_cutoff, double *out, uint64_t out_ld);

/*
 * Threshold join: every pair (query i, candidate j) with score(i, j) >= score_cutoff, as CSR -- the question of record linkage and
 * deduplication, "which pairs score at least 0.85" (found by dlsym, like the search calls and cdist: the ABI version stays 1.7, and
 * strsim_measure_supported does not describe these two entry points).  `scorer` is STRSIM_INDEL (8) or STRSIM_TOKEN_SORT_RATIO
 * (14), extract's two; score(i, j) is bit for bit what strsim_pairs_device(scorer, queries[i], candidates[j]) returns.  With
 * STRSIM_JOIN_UPPER in `flags` only pairs with j > i are reported: pass one column as both sides for a self-join.
 *
 * Output.  out_indptr[0] = 0, out_indptr[i + 1] - out_indptr[i] is the number of hits of query i, and they sit at out_index /
 * out_score[out_indptr[i] .. out_indptr[i + 1]) in ASCENDING CANDIDATE INDEX: one canonical order, which does not depend on how the
 * work was split or visited and compares equal run to run.
 * Capacity.  *out_nnz (HOST memory) and all of out_indptr are always written, and exact.  out_index and out_score (capacity
 * elements each) are written iff nnz <= capacity; otherwise not one element of either is touched and the call still returns
 * STRSIM_OK: the caller compares *out_nnz with capacity, allocates and calls again.  capacity == 0 with NULL out_index / out_score
 * is the count-only form.
 * score_cutoff = -INFINITY or 0.0 reports every pair (cdist as CSR), a cutoff above 1.0 nothing (no sweep is launched); NaN is
 * STRSIM_ERR_ARG.
 *
 * q_rows <= 2^32 - 1, c_rows <= 2^32 - 2; q_rows == 0 writes out_indptr[0] = 0 and *out_nnz = 0, c_rows == 0 gives all-zero counts.
 * An unknown scorer, unknown flag bits, a NULL buffer of a non-empty side, a NULL out_nnz or out_indptr, a non-zero capacity with a
 * NULL output: STRSIM_ERR_ARG.  The arguments are checked first, the context last (a NULL ctx is STRSIM_ERR_ARG too): no argument
 * error needs a device.  Nulls are not seen here: a caller drops null candidates and maps the indices back.
 *
 * Device-resident: the same column layout as strsim_pairs_device.  Strings of at most 32 ASCII bytes are swept one query per lane
 * in length order, visiting only the candidate lengths whose best possible score can reach the cutoff -- once to count the hits of
 * every row, then, when they fit, once more to store them; the rows are then sorted by candidate index.  Every pair with a longer or
 * non-ASCII side goes through strsim_pairs_device(STRSIM_INDEL) (that string as the literal); those scores are kept for the second
 * pass up to 128 MB, beyond that both passes make the calls.  Scorer 14 first
 * normalises both columns on the device, as strsim_extract_device does.
 * Waits for the stream: scorer 14 waits once for the bounds of its columns; every call waits once for a read-back of how many
 * strings fall outside the one-query-per-lane class and once for nnz.  Without such strings it then returns with the fill and the
 * sort enqueued: out_index / out_score are complete after strsim_ctx_synchronize(), or in stream order.  With them it runs those
 * pairs through strsim_pairs_device batch by batch, each of which waits for the stream.  Scratch the context cannot reserve is
 * STRSIM_ERR_OOM.
 */
#define STRSIM_JOIN_UPPER 1u /* report only pairs with j > i (self-join / dedup: pass the same column twice) */
STRSIM_API int strsim_join_device(strsim_ctx_t *ctx, int scorer,
                                  const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                  const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                  double score_cutoff, uint32_t flags, uint64_t capacity,
                                  uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz);

/* The same with HOST-RESIDENT buffers (the column layout of strsim_pairs_host, every output included); synchronous. */
STRSIM_API int strsim_join_host(strsim_ctx_t *ctx, int scorer,
                                const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                double score_cutoff, uint32_t flags, uint64_t capacity,
                                uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz);

/*
 * Threshold join by the five reference measures: every pair (query i, candidate j) with score(i, j) >= min_score, as CSR -- "every
 * pair of names with Jaro-Winkler >= 0.9" without the N x M matrix of cdist and without best_match's limit of 16 candidates (found
 * by dlsym, like strsim_join_*: the ABI version stays 1.7 and strsim_measure_supported does not describe these two entry points).
 * `measure` is one of the reference measures, STRSIM_LEVENSHTEIN (0) .. STRSIM_SORENSEN_DICE (4); score(i, j) is bit for bit what
 * strsim_pairs_device(measure, queries[i], candidates[j]) returns, and a hit is the f64 comparison score >= min_score.
 *
 * Everything else is the contract of strsim_join_device, word for word: STRSIM_JOIN_UPPER in `flags` keeps only j > i; the result
 * is CSR with every row in ascending candidate index; *out_nnz (host memory) and all of out_indptr are always written, and exact;
 * out_index and out_score (capacity elements each) are written iff nnz <= capacity, otherwise not one element of either is touched
 * and the call still returns STRSIM_OK; capacity == 0 with NULL out_index / out_score is the count-only form.  min_score = -INFINITY
 * or 0.0 reports every pair, a value above 1.0 nothing (no sweep is launched, one clear of out_indptr is enqueued); NaN is
 * STRSIM_ERR_ARG.  The limits on the rows, the argument errors and their order (arguments first, the context last) and the waits
 * are those of strsim_join_device too.
 *
 * Device-resident: strings of at most 32 ASCII bytes are swept one query per lane in length order, visiting only the candidate
 * lengths at which the measure's own best score for the two lengths reaches min_score (a table of 33 x 33 bits the host builds per
 * call and passes as a kernel argument) -- once to count, then, when the hits fit, once more to store them; the rows are then
 * sorted by candidate index.  Every pair with a longer or non-ASCII side goes through strsim_pairs_device(measure) with that string
 * as the literal, as in strsim_join_device.
 */
STRSIM_API int strsim_match_join_device(strsim_ctx_t *ctx, int measure,
                                        const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                        const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                        double min_score, uint32_t flags, uint64_t capacity,
                                        uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz);

/* The same with HOST-RESIDENT buffers (the column layout of strsim_pairs_host, every output included); synchronous. */
STRSIM_API int strsim_match_join_host(strsim_ctx_t *ctx, int measure,
                                      const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                      const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                      double min_score, uint32_t flags, uint64_t capacity,
                                      uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz);

/*
 * Connected components of a CSR graph: one label per row -- the last stage of deduplication, "these 7 spellings are the same
 * customer" (found by dlsym, like strsim_join_*: the ABI version stays 1.7 and strsim_measure_supported does not describe these
 * entry points).  The nnz edges (i, index[e]), e in [indptr[i], indptr[i + 1]), are read as UNDIRECTED: the upper-only CSR of a
 * STRSIM_JOIN_UPPER self-join, a lower-only one and a two-sided one give the same answer; duplicate edges and self-loops are harmless.
 *
 * Output.  out_root[v] is the smallest row of v's component: canonical, the same run to run.  out_cluster[v] (may be NULL) is the
 * number of roots below out_root[v]: the clusters are numbered 0 .. count - 1 in order of their first member.  *out_count (HOST
 * memory) is the number of components; a row without an edge is a component of one.
 *
 * rows <= 2^32 - 1.  rows == 0 writes *out_count = 0 and touches no device memory; nnz == 0 gives the identity (one launch, no
 * wait).  A NULL indptr or out_count, a NULL out_root with rows > 0, a NULL index with nnz > 0, too many rows: STRSIM_ERR_ARG; the
 * arguments are checked first, the context last (a NULL ctx is STRSIM_ERR_ARG too): no argument error needs a device.  An
 * index[e] >= rows is skipped by the kernel and counted; the call then returns STRSIM_ERR_ARG with "index out of range" (the labels
 * of the remaining edges are written).  indptr is assumed non-decreasing from 0 to nnz; whatever it holds, no access leaves the
 * caller's buffers (csrc/strsim_components.h has the argument).
 *
 * Device-resident: init, link (one lane per edge, hook-to-smaller with a compare-and-swap; no lane waits for another), compress,
 * a scan of the root flags and the rank: seven launches and one 16-byte copy for every graph with nnz > 0, then the call's one
 * wait for the stream (the count and the bad-index word come back together).  Scratch (20 bytes a row) the context cannot reserve
 * is STRSIM_ERR_OOM.
 */
STRSIM_API int strsim_components_device(strsim_ctx_t *ctx, uint64_t rows, const uint64_t *indptr, const uint32_t *index, uint64_t nnz,
                                        uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count);

/* The same with HOST-RESIDENT buffers; synchronous. */
STRSIM_API int strsim_components_host(strsim_ctx_t *ctx, uint64_t rows, const uint64_t *indptr, const uint32_t *index, uint64_t nnz,
                                      uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count);

/*
 * The duplicate groups of one column: the STRSIM_JOIN_UPPER self-join of the column with itself at min_score, followed by
 * strsim_components_device on its CSR.  The pairs live in a grow-only buffer of the context and never reach the host.  `measure`
 * 0 .. 4 runs strsim_match_join_device, STRSIM_INDEL (8) and STRSIM_TOKEN_SORT_RATIO (14) run strsim_join_device; any other id is
 * STRSIM_ERR_ARG.  The join is made with 4 * rows + 1024 slots and, when the hits do not fit, once more with exactly nnz.
 * Components chain: a ~ b and b ~ c put a and c in one cluster even where a and c do not match each other.
 *
 * out_root, out_cluster (may be NULL) and *out_count (HOST memory) are those of strsim_components_device; *out_nnz (HOST memory,
 * may be NULL) is the number of pairs of the self-join.  NaN and the range of min_score follow the join: above 1.0 nothing matches
 * (the identity), -INFINITY or 0.0 gives one cluster, NaN is STRSIM_ERR_ARG.  rows <= 2^32 - 2; rows == 0 writes *out_count = 0.
 * The arguments are checked first, the context last.  Waits: the join's, then the one of the components.
 */
STRSIM_API int strsim_cluster_device(strsim_ctx_t *ctx, int measure, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                                     double min_score, uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz);

/* The same with HOST-RESIDENT buffers; synchronous. */
STRSIM_API int strsim_cluster_host(strsim_ctx_t *ctx, int measure, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                                   double min_score, uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz);

/*
 * Threshold join by q-gram similarity: every pair (query i, candidate j) whose q-gram score is >= min_score, as CSR -- "which rows
 * of this column look like which rows of that one, at trigram similarity 0.8 or better" (found by dlsym, like strsim_join_*: the
 * ABI version stays 1.7, there is no new measure id and strsim_measure_supported does not describe these entry points).  `kind`,
 * `q` and `qflags` are the kind, q and flags of strsim_qgram_device (STRSIM_QGRAM_JACCARD .. _COSINE, 1 .. 3, STRSIM_QGRAM_SET);
 * score(i, j) is bit for bit what strsim_qgram_device(kind, q, qflags, queries[i], candidates[j]) returns, and a hit is the f64
 * comparison score >= min_score.
 *
 * Everything else is the contract of strsim_match_join_device, word for word: STRSIM_JOIN_UPPER in `flags` keeps only j > i; the
 * result is CSR with every row in ascending candidate index; *out_nnz (host memory) and all of out_indptr are always written, and
 * exact; out_index and out_score (capacity elements each) are written iff nnz <= capacity, otherwise not one element of either is
 * touched and the call still returns STRSIM_OK; capacity == 0 with NULL out_index / out_score is the count-only form.  min_score =
 * -INFINITY or 0.0 reports every pair, a value above 1.0 nothing (no sweep is launched, one clear of out_indptr is enqueued); NaN
 * is STRSIM_ERR_ARG.  kind, q and qflags are checked first, in strsim_qgram_device's words, then the arguments of
 * strsim_match_join_device in its order, the context last: no argument error needs a device.
 *
 * Device-resident: strings of at most 32 ASCII bytes are swept one query per lane in length order.  In multiset mode only the
 * candidate lengths are visited at which the kind's own best score for the two gram counts reaches min_score (Jaccard,
 * Sorensen-Dice, cosine; the overlap coefficient reaches 1.0 at every pair of lengths and is never pruned).  In set mode the counts
 * are those of distinct grams, which lengths do not bound: every length with a gram is visited.  Every pair with a longer or
 * non-ASCII side goes through strsim_qgram_device's kernels with that string as the literal; those internal calls leave
 * strsim_ctx_last_wave_rows as the caller's last pairwise call set it.
 */
STRSIM_API int strsim_qgram_join_device(strsim_ctx_t *ctx, int kind, uint32_t q, uint32_t qflags,
                                        const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                        const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                        double min_score, uint32_t flags, uint64_t capacity,
                                        uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz);

/* The same with HOST-RESIDENT buffers (the column layout of strsim_pairs_host, every output included); synchronous. */
STRSIM_API int strsim_qgram_join_host(strsim_ctx_t *ctx, int kind, uint32_t q, uint32_t qflags,
                                      const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                      const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                      double min_score, uint32_t flags, uint64_t capacity,
                                      uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz);

/*
 * The duplicate groups of one column by q-gram similarity: strsim_cluster_device with the STRSIM_JOIN_UPPER self-join made by
 * strsim_qgram_join_device(kind, q, qflags).  Outputs, the range of min_score, the limits and the waits are strsim_cluster_device's;
 * kind, q and qflags are checked first, then its remaining arguments in its order, the context last.
 */
STRSIM_API int strsim_qgram_cluster_device(strsim_ctx_t *ctx, int kind, uint32_t q, uint32_t qflags,
                                           const uint32_t *offsets, const uint8_t *values, uint64_t rows, double min_score,
                                           uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz);

/* The same with HOST-RESIDENT buffers; synchronous. */
STRSIM_API int strsim_qgram_cluster_host(strsim_ctx_t *ctx, int kind, uint32_t q, uint32_t qflags,
                                         const uint32_t *offsets, const uint8_t *values, uint64_t rows, double min_score,
                                         uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz);

/*
 * Join by integer edit distance: every pair (query i, candidate j) with d(i, j) <= max_distance, as CSR -- "which rows are within
 * two edits of which" (found by dlsym, like strsim_join_*: the ABI version stays 1.7, there is no new measure id and
 * strsim_measure_supported does not describe these entry points).  `kind` is one of STRSIM_EDIT_*: d(i, j) is exactly what
 * strsim_distance_device(STRSIM_LEVENSHTEIN or STRSIM_OSA, ..., STRSIM_DISTANCE_UNBOUNDED) returns for the pair, and for
 * STRSIM_EDIT_DAMERAU what strsim_damerau_distance_device(..., STRSIM_DISTANCE_UNBOUNDED) returns: the unrestricted
 * Damerau-Levenshtein distance, the one of the three that is a metric.  max_distance = 0 is the exact-duplicate join,
 * STRSIM_DISTANCE_UNBOUNDED reports every pair.  Any other kind is STRSIM_ERR_ARG.
 *
 * Everything else is the contract of strsim_match_join_device, word for word, with out_distance (uint32, capacity elements) where
 * out_score stands: STRSIM_JOIN_UPPER in `flags` keeps only j > i; the result is CSR with every row in ascending candidate index;
 * *out_nnz (host memory) and all of out_indptr are always written, and exact; out_index and out_distance are written iff
 * nnz <= capacity, otherwise not one element of either is touched and the call still returns STRSIM_OK; capacity == 0 with NULL
 * out_index / out_distance is the count-only form.  The kind is checked first, then the arguments of strsim_match_join_device in
 * its order, the context last: no argument error needs a device.
 *
 * Device-resident: strings of at most 32 ASCII bytes are swept one query per lane in length order; d >= | |a| - |b| | by all three
 * measures, so only the candidate lengths within max_distance of a query's are visited.  Levenshtein and OSA run their
 * bit-parallel column.  Damerau-Levenshtein runs the OSA column and decides by it wherever it can (osa <= 2: d = osa; osa >
 * 2 max_distance: no hit) and runs its cell DP only for the rest: at max_distance <= 1 never.  Every pair with a longer or
 * non-ASCII side goes through strsim_distance_device / strsim_damerau_distance_device at max_distance with that string as the
 * literal; those internal calls leave strsim_ctx_last_wave_rows as the caller's last pairwise call set it.  The hits travel as
 * f64 inside the call: a context-owned buffer of min(capacity, q_rows * c_rows) doubles.
 */
enum { STRSIM_EDIT_LEVENSHTEIN = 0, STRSIM_EDIT_OSA = 1, STRSIM_EDIT_DAMERAU = 2 };

STRSIM_API int strsim_distance_join_device(strsim_ctx_t *ctx, int kind,
                                           const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                           const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                           uint32_t max_distance, uint32_t flags, uint64_t capacity,
                                           uint64_t *out_indptr, uint32_t *out_index, uint32_t *out_distance, uint64_t *out_nnz);

/* The same with HOST-RESIDENT buffers (the column layout of strsim_pairs_host, every output included); synchronous. */
STRSIM_API int strsim_distance_join_host(strsim_ctx_t *ctx, int kind,
                                         const uint32_t *q_offsets, const uint8_t *q_values, uint64_t q_rows,
                                         const uint32_t *c_offsets, const uint8_t *c_values, uint64_t c_rows,
                                         uint32_t max_distance, uint32_t flags, uint64_t capacity,
                                         uint64_t *out_indptr, uint32_t *out_index, uint32_t *out_distance, uint64_t *out_nnz);

/*
 * The duplicate groups of one column by edit distance: strsim_cluster_device with the STRSIM_JOIN_UPPER self-join made by
 * strsim_distance_join_device(kind, max_distance): rows within max_distance edits are linked and the links chain ("a" ~ "b" ~ "c"
 * is one group even when "a" and "c" are further apart).  Outputs, the limits and the waits are strsim_cluster_device's;
 * STRSIM_DISTANCE_UNBOUNDED gives one cluster, as min_score = -INFINITY does there.  The kind is checked first, then the remaining
 * arguments in strsim_cluster_device's order, the context last.
 */
STRSIM_API int strsim_distance_cluster_device(strsim_ctx_t *ctx, int kind, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                                              uint32_t max_distance, uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count,
                                              uint64_t *out_nnz);

/* The same with HOST-RESIDENT buffers; synchronous. */
STRSIM_API int strsim_distance_cluster_host(strsim_ctx_t *ctx, int kind, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                                            uint32_t max_distance, uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count,
                                            uint64_t *out_nnz);

/* Row partition used to shard a column over `n` GPUs/ranks: the reference's split_offsets
 * (strsim.rs:21-39).  Writes n (offset,len) pairs into out_offset_len[2*n]. */
STRSIM_API void strsim_split_offsets(uint64_t len, uint64_t n, uint64_t *out_offset_len);

/*
 * Kernel timing for roofline accounting.  When enabled, every strsim_pairs_device() brackets its
 * dominant (lane-per-pair) kernel and its wave-per-pair kernel with hipEvents on the context's stream.
 * strsim_ctx_timing_read() synchronises and returns the accumulated milliseconds and launch counts
 * since the last read, then resets them.
 */
STRSIM_API int strsim_ctx_timing_enable(strsim_ctx_t *ctx, int enable);
STRSIM_API int strsim_ctx_timing_read(strsim_ctx_t *ctx, double *lane_kernel_ms, uint64_t *lane_kernel_launches,
                           double *wave_kernel_ms, uint64_t *wave_kernel_launches);

/* Offsets of a column from its string LENGTHS, on the device: offsets[0] = 0, offsets[i + 1] = offsets[i] + lengths[i]
 * (lengths: `rows` bytes on the device, 16-byte aligned; offsets: rows + 1 words).  Asynchronous on the context's stream.
 * For a host that holds strings as views / (pointer, length) pairs (Polars' Utf8View, the layout the reference iterates at
 * strsim.rs:46-47) and ships one length byte per row over PCIe instead of a u32 offset; strings of at most 255 bytes, at
 * most STRSIM_OFFSETS_FROM_LENGTHS_MAX_ROWS rows per call (= floor((2^32 - 1) / 255): the 32-bit offsets cannot wrap whatever
 * the lengths are; more rows: STRSIM_ERR_ARG).  The result is what strsim_pairs_device() takes as a_offsets / b_offsets. */
#define STRSIM_OFFSETS_FROM_LENGTHS_MAX_ROWS 16843009u
STRSIM_API int strsim_offsets_from_lengths(strsim_ctx_t *ctx, const uint8_t *lengths, uint64_t rows, uint32_t *offsets);

/* A column from Utf8View slots, on the device (ABI 1.4; SURVEY 8 f1: the layout the reference iterates, strsim.rs:46-47).  `views`:
 * rows Arrow Utf8View slots of 16 bytes each, 16-byte aligned, as the engine holds them -- a u32 length, then either the string
 * itself (length <= 12) or its first four bytes, a u32 buffer index and a u32 offset -- with ONE thing changed by the host on the
 * way: a slot whose string does not fit it (length > 12) carries in its last word the string's offset in `long_values`, the bytes
 * of those strings as the host has shipped them (any order, gaps allowed; the buffer index is ignored).  A null slot is shipped as
 * length 0.  Writes offsets[rows + 1] and the packed values (their size, the sum of the lengths, is the host's to know: it has
 * seen every length) -- what strsim_pairs_device() takes.  Asynchronous on the context's stream, two launches; the packed size of
 * one call must fit 32-bit offsets, at most 33 554 432 rows per call.  Reference counterpart: none (the reference reads the views
 * in place); this is what lets a host with few cycles to spare -- the engine-parallel mode packs on the calling thread alone --
 * hand a String column over with a streaming copy instead of a gather. */
STRSIM_API int strsim_column_from_views(strsim_ctx_t *ctx, const void *views, uint64_t rows, const uint8_t *long_values,
                                        uint32_t *offsets, uint8_t *values);
/* The same with the extents stated (ABI 1.5): `long_values` holds long_bytes bytes, `values` has room for values_bytes.  A slot
 * whose string would be read from outside long_values (or whose long_values is NULL), or written outside values -- a malformed
 * column: the slots are the host's to get right -- is NOT copied (its offsets are still written) and counted in *malformed, a
 * u32 on the device that the caller has zeroed (NULL: not counted): a bad slot cannot fault the GPU.  Sums of lengths beyond
 * 2^32 - 1 put every later row out of range instead of wrapping.  strsim_column_from_views() is this call with the extents
 * "not stated" (a NULL long_values still skips every slot beyond 12 bytes). */
STRSIM_API int strsim_column_from_views_bounded(strsim_ctx_t *ctx, const void *views, uint64_t rows, const uint8_t *long_values,
                                                uint64_t long_bytes, uint32_t *offsets, uint8_t *values, uint64_t values_bytes,
                                                uint32_t *malformed);

/* Close the gaps between up to STRSIM_COMPACT_MAX_SEGMENTS byte segments on the device, one launch on the context's stream:
 * dst[dst_off[k] .. + bytes[k]) = src[src_off[k] .. + bytes[k]) for k < nseg; src and dst are distinct device buffers, the three
 * arrays are host memory (read before the call returns).  For a host that packs a column's values with several threads in ONE
 * pass -- each thread into its own segment of a staging buffer, no common prefix, one length byte per row (see
 * strsim_offsets_from_lengths) -- and ships the buffer as it lies: the plugin layer does (reference counterpart: none; the
 * reference iterates the views in place, strsim.rs:46-47). */
#define STRSIM_COMPACT_MAX_SEGMENTS 32
STRSIM_API int strsim_compact_segments(strsim_ctx_t *ctx, const uint8_t *src, uint8_t *dst, const uint64_t *src_off,
                                       const uint64_t *dst_off, const uint64_t *bytes, int nseg);

/* For a caller that keeps several calls in flight on the context's stream and learns of their completion by its own means
 * (an event recorded on strsim_ctx_stream() behind each call): retire the OLDEST pending call only -- what
 * strsim_ctx_synchronize() does for all of them, without waiting for the younger ones.  The caller guarantees that the
 * oldest call's kernels have completed; the library checks it (the call's status block carries a ticket the device writes
 * last) and returns STRSIM_ERR_ARG, leaving the call pending, when they have not -- an event recorded on any OTHER stream
 * than strsim_ctx_stream() proves nothing about this context's kernels.  If that call held strings longer than STRSIM_WAVE_PATH_MAX_BYTES, their second
 * pass is launched and waited for here (strsim_ctx_last_long_rows() tells).  Reference counterpart: none -- the reference's
 * rayon loop (strsim.rs:72-100) has no device queue; this is what lets the plugin overlap H2D of slice k+1, the kernels of
 * slice k and the D2H of slice k-1. */
STRSIM_API int strsim_ctx_retire_oldest(strsim_ctx_t *ctx);

/* Rows the last completed strsim_pairs_device() on this context routed to the wave-per-pair kernel
 * (valid after strsim_ctx_synchronize()). */
STRSIM_API uint64_t strsim_ctx_last_wave_rows(strsim_ctx_t *ctx);

/* Rows of the calls retired by the last strsim_ctx_synchronize() / strsim_ctx_retire_oldest() that held a string longer than
 * STRSIM_WAVE_PATH_MAX_BYTES: their results were written by the second pass that synchronize runs, i.e. AFTER anything
 * the caller enqueued on the stream behind the call (a caller that copies results out early re-copies when > 0). */
STRSIM_API uint64_t strsim_ctx_last_long_rows(strsim_ctx_t *ctx);

/* Rows of the calls retired by the last strsim_ctx_synchronize() / strsim_ctx_retire_oldest() whose results were written by a
 * pass launched from there -- the slow-row kernels of a one-launch call that did hold such rows, and the long-string pass --
 * i.e. AFTER anything the caller enqueued on the stream behind the call (a caller that copied results out early copies again
 * when this is > 0).  >= strsim_ctx_last_long_rows(). */
STRSIM_API uint64_t strsim_ctx_last_late_rows(strsim_ctx_t *ctx);

/* Kernels and device copies this context has enqueued for pair calls since it was created (a call of a column whose rows
 * all fit the one-pair-per-lane kernel adds 1; a call with all kernels up front 5; introspection for tests and benches). */
STRSIM_API uint64_t strsim_ctx_enqueued_ops(strsim_ctx_t *ctx);

/* ---- the gather of the result shards over RCCL (ABI 1.5) --------------------------------------------------------------------
 * Rows are independent, so N processes -- one per GPU -- each run strsim_pairs_device on the shard strsim_split_offsets(rows, N)
 * gives them (the reference's own partition, strsim.rs:21-39) with no data-path collective; the one exchange step of the path is
 * the gather of the f64 result shards onto a root rank (reference counterpart: the threads' chunks collected into one
 * Float64Chunked, strsim.rs:98-104).  These four calls are that step for a host that binds this header (a Rust shim: INTEGRATION.md):
 *   rank 0:      strsim_gather_unique_id(id)            -- and hands the 128 bytes to the other ranks by whatever means it has
 *   every rank:  strsim_gather_create(ctx, id, N, rank, &g)   (collective: returns when all N ranks have called it)
 *   every step:  strsim_gather_f64(g, shard, column, rows, root)   -- enqueued on the context's stream behind the kernels
 * `shard`: this rank's rows of the result column (device memory, split_offsets(rows, N)[rank] of them); `column`: the whole
 * column on the root (device memory, `rows` doubles; ignored elsewhere).  Every peer's shard travels point to point into the root
 * (ncclSend / ncclRecv in one group: xGMI is point-to-point, seven links into the root at N = 8), the root's own shard is a device
 * copy.  RCCL is resolved at first use (a copy the process already holds, else librccl.so.1 from the loader's path) and is not a
 * link-time dependency of the library; without it these calls fail with STRSIM_ERR_NO_DEVICE and nothing else is affected.
 * STRSIM_RCCL_LIB=<path> names the library to use instead (read once per process). */
#define STRSIM_GATHER_ID_BYTES 128
typedef struct strsim_gather strsim_gather_t;
STRSIM_API int strsim_gather_unique_id(uint8_t id[STRSIM_GATHER_ID_BYTES]);
STRSIM_API int strsim_gather_create(strsim_ctx_t *ctx, const uint8_t id[STRSIM_GATHER_ID_BYTES], int world_size, int rank,
                                    strsim_gather_t **out);
STRSIM_API int strsim_gather_f64(strsim_gather_t *g, const double *shard, double *column, uint64_t total_rows, int root);
/* The same over an explicit partition (ABI 1.6): ranges = uint64[2 * N], rank r holds rows [ranges[2r], ranges[2r] + ranges[2r+1])
 * of the column -- for a host whose shards are not split_offsets' (a root that takes a smaller share because it also assembles the
 * column: a named deviation from strsim.rs:21-39).  The same array on every rank; overlapping ranges are refused. */
STRSIM_API int strsim_gather_f64_ranges(strsim_gather_t *g, const double *shard, double *column, const uint64_t *ranges, int root);
/* How many ranks the RCCL communicator of `g` itself holds (ncclCommCount): the answer to "did RCCL form the world I think it did"
 * that does not go through the caller's own bookkeeping (ABI 1.6). */
STRSIM_API int strsim_gather_comm_count(strsim_gather_t *g, int *count);
STRSIM_API void strsim_gather_destroy(strsim_gather_t *g);

/*
 * Lossless 16-bit transport codec for result columns (csrc/strsim_codec.hip).  A similarity of two strings of at
 * most `max_chars` characters takes few distinct values (max_chars = 32: 325 / 22 856 / 57 359 / 631 / 631 for the
 * five measures); the codec ships the 16-bit rank of each value instead of 8 bytes -- 4x less traffic on the
 * point-to-point xGMI link of a gather -- and decodes bit-exactly.  Values outside the table (rows with longer
 * strings) are coded 0xFFFF and reported as (row, value) exceptions.  All buffers are device memory of the
 * context's GPU; calls are asynchronous on the context's stream.
 */
typedef struct strsim_codec strsim_codec_t;
/* Fails with STRSIM_ERR_ARG when the value set does not fit 16 bits (e.g. Jaro with max_chars = 128). */
STRSIM_API int strsim_codec_create(strsim_ctx_t *ctx, int measure, uint32_t max_chars, strsim_codec_t **out);
STRSIM_API void strsim_codec_destroy(strsim_codec_t *codec);
STRSIM_API uint32_t strsim_codec_entries(const strsim_codec_t *codec);
/* vals[n] -> codes[n]; *exc_count (device) = number of exceptions, the first exc_cap of them in exc_rows/exc_vals. */
STRSIM_API int strsim_codec_encode(strsim_ctx_t *ctx, const strsim_codec_t *codec, const double *vals, uint64_t n,
                                   uint16_t *codes, uint32_t *exc_count, uint32_t *exc_rows, double *exc_vals,
                                   uint32_t exc_cap);
/* codes[n] -> out[n]; rows coded 0xFFFF are left untouched. */
STRSIM_API int strsim_codec_decode(strsim_ctx_t *ctx, const strsim_codec_t *codec, const uint16_t *codes, uint64_t n,
                                   double *out);
/* Packed transport of the same codes: strsim_codec_bits() bits per row (the smallest b with 2^b > entries; the
 * all-ones code is the escape), 64 / bits rows per 64-bit word: 9.14 bits per row for Levenshtein (325 values),
 * 10.67 for Jaccard / Dice (631).  words[strsim_codec_packed_words(codec, n)]; exceptions as in strsim_codec_encode. */
STRSIM_API uint32_t strsim_codec_bits(const strsim_codec_t *codec);
STRSIM_API uint64_t strsim_codec_packed_words(const strsim_codec_t *codec, uint64_t n);
STRSIM_API int strsim_codec_encode_packed(strsim_ctx_t *ctx, const strsim_codec_t *codec, const double *vals, uint64_t n,
                                          uint64_t *words, uint32_t *exc_count, uint32_t *exc_rows, double *exc_vals,
                                          uint32_t exc_cap);
STRSIM_API int strsim_codec_decode_packed(strsim_ctx_t *ctx, const strsim_codec_t *codec, const uint64_t *words, uint64_t n,
                                          double *out);
/* out[row_base + exc_rows[i]] = exc_vals[i] for i < count. */
STRSIM_API int strsim_codec_patch(strsim_ctx_t *ctx, double *out, uint64_t row_base, const uint32_t *exc_rows,
                                  const double *exc_vals, uint32_t count);

/* The same with the count read on the device: exc_count / exc_rows / exc_vals are another rank's exception block as it
 * arrived with the gathered codes (strsim_amd/distributed.py).  A count above exc_cap (the sender had more exceptions than
 * the block holds: the column is incomplete) increments *overflow (device memory). */
STRSIM_API int strsim_codec_patch_indirect(strsim_ctx_t *ctx, double *out, uint64_t row_base, const uint32_t *exc_count,
                                           const uint32_t *exc_rows, const double *exc_vals, uint32_t exc_cap,
                                           uint32_t *overflow);

/* The root's side of a gather in ONE launch: `buf` holds nseg segments seg_stride_bytes apart, segment r = rank r's codes (packed:
 * strsim_codec_encode_packed's words; else 16-bit codes) followed, code_bytes into the segment, by its exception block -- count
 * (u32, 16-byte field), exc_cap rows (u32), exc_cap values (f64).  Rows r * chunk_rows .. (last segment: last_rows of them) of `out`
 * are decoded and the exceptions written in; a count above exc_cap increments *overflow (device).  Replaces one
 * strsim_codec_decode(_packed) + one strsim_codec_patch_indirect launch per peer (strsim_amd/distributed.py). */
STRSIM_API int strsim_codec_decode_gathered(strsim_ctx_t *ctx, const strsim_codec_t *codec, const void *buf, uint64_t seg_stride_bytes,
                                            uint32_t nseg, uint64_t chunk_rows, uint64_t last_rows, int packed, uint64_t code_bytes,
                                            uint32_t exc_cap, double *out, uint32_t *overflow);
/* The same over segments first_seg .. nseg - 1 only (ABI 1.5): the root of a gather has no reason to code and decode its OWN shard --
 * it copies its f64 results into `out` and decodes the peers' segments (first_seg = 1: an eighth of the decode and the whole
 * encode off the rank that every step waits for, profiles/r5_root_rehearsal.txt).  Row r * chunk_rows is still segment r's first. */
STRSIM_API int strsim_codec_decode_gathered_from(strsim_ctx_t *ctx, const strsim_codec_t *codec, const void *buf, uint64_t seg_stride_bytes,
                                                 uint32_t first_seg, uint32_t nseg, uint64_t chunk_rows, uint64_t last_rows, int packed,
                                                 uint64_t code_bytes, uint32_t exc_cap, double *out, uint32_t *overflow);

#define STRSIM_LANE_PATH_MAX_BYTES 32u   /* lane-per-pair kernels: both strings <= 32 bytes, ASCII */
#define STRSIM_WAVE_PATH_MAX_BYTES 1024u /* wave-per-pair kernels: both strings <= 1024 bytes, any UTF-8 */

#ifdef __cplusplus
}
#endif
#endif /* STRSIM_AMD_H */
