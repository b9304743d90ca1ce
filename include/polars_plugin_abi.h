/*
 * polars_plugin_abi.h -- the Polars expression-plugin C ABI exported by libpolars_strsim_amd.so.
 *
 * These are the symbols the reference's five `#[polars_expr(output_type=Float64)]` functions expand to
 * (reference src/expressions/mod.rs:8-31; macro = pyo3-polars-derive 0.11.0, FFI structs = polars-ffi
 * 0.43.1 `version_0`, pins in the reference's Cargo.lock:588-589,855-856,874-875).  Polars dlopen()s the one
 * shared library found in the plugin package directory (`plugin_path=Path(__file__).parent`, reference
 * polars_strsim/__init__.py:11-16), checks the version symbol and calls `_polars_plugin_<name>` with the
 * input Series exported over the Arrow C Data Interface.  Neither crate's source is vendored in the
 * reference tree: the layouts below are restated from the published 0.43.1 / 0.11.0 sources and are
 * "verify on first contact" (SURVEY.md 8b); tests/test_plugin_abi_gpu.py and tests/test_abi_symbols.py drive them with
 * pyarrow as the host (strsim_amd/arrow_host.py).
 *
 * Ownership (polars-ffi `import_series` / `export_series`): the callee owns every input SeriesExport and
 * every ArrowArray in it -- it calls each array's release and then the SeriesExport's release, once.  On
 * success it writes a fully formed SeriesExport into *return_value (the host imports the arrays by
 * bitwise copy and then calls return_value->release).  On failure *return_value is left untouched and
 * the message is available from _polars_plugin_get_last_error_message() on the same thread.
 */
#ifndef POLARS_PLUGIN_ABI_H
#define POLARS_PLUGIN_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define POLARS_PLUGIN_API __attribute__((visibility("default")))
#else
#define POLARS_PLUGIN_API
#endif

/* ---- Arrow C Data Interface (https://arrow.apache.org/docs/format/CDataInterface.html) ---- */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4

struct ArrowSchema {
    const char *format;
    const char *name;
    const char *metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema **children;
    struct ArrowSchema *dictionary;
    void (*release)(struct ArrowSchema *);
    void *private_data;
};

struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void **buffers;
    struct ArrowArray **children;
    struct ArrowArray *dictionary;
    void (*release)(struct ArrowArray *);
    void *private_data;
};
#endif

/* ---- polars-ffi 0.43.1 version_0 ---- */
typedef struct SeriesExport {
    struct ArrowSchema *field;   /* name + dtype of the Series */
    struct ArrowArray **arrays;  /* `len` chunks */
    size_t len;
    void (*release)(struct SeriesExport *);
    void *private_data;
} SeriesExport;

typedef struct CallerContext {
    uint64_t bitflags; /* bit 0 = PARALLEL: the engine is already inside a parallel region (reference strsim.rs:53) */
} CallerContext;

#define POLARS_PLUGIN_VERSION_MAJOR 0u
#define POLARS_PLUGIN_VERSION_MINOR 1u /* minor 1 = call form carrying the CallerContext */

POLARS_PLUGIN_API uint32_t _polars_plugin_get_version(void);                  /* (major << 16) | minor */
POLARS_PLUGIN_API const char *_polars_plugin_get_last_error_message(void);    /* thread-local, NUL-terminated */

#define POLARS_PLUGIN_DECLARE(name)                                                                                  \
    POLARS_PLUGIN_API void _polars_plugin_##name(SeriesExport *inputs, size_t n_inputs, const uint8_t *kwargs,       \
                                                 size_t kwargs_len, SeriesExport *return_value, CallerContext *ctx); \
    POLARS_PLUGIN_API void _polars_plugin_field_##name(struct ArrowSchema *input_fields, size_t n_fields,            \
                                                       struct ArrowSchema *return_value);

/* reference src/expressions/mod.rs:8-11, :13-16, :18-21, :23-26, :28-31 */
POLARS_PLUGIN_DECLARE(levenshtein)
POLARS_PLUGIN_DECLARE(jaro)
POLARS_PLUGIN_DECLARE(jaro_winkler)
POLARS_PLUGIN_DECLARE(jaccard)
POLARS_PLUGIN_DECLARE(sorensen_dice)
/* Not in the reference: optimal string alignment -- the restricted Damerau-Levenshtein similarity (adjacent transpositions count
 * one edit, no substring is edited twice), STRSIM_OSA of strsim_amd.h.  Same inputs, output (Float64 named after input 0), nulls
 * and literal broadcast as the five above. */
POLARS_PLUGIN_DECLARE(osa)
/* Not in the reference: bounded integer edit distances (strsim_distance_host of strsim_amd.h), Levenshtein and OSA.  Inputs 0 and 1
 * as above (shape rule, literal broadcast, nulls); an optional input 2 is max_distance, a length-1 non-null UInt32 series (rows with
 * a larger distance hold max_distance + 1).  Output: one UInt32 chunk named after input 0.  These calls bypass the small-call
 * combiner. */
POLARS_PLUGIN_DECLARE(levenshtein_distance)
POLARS_PLUGIN_DECLARE(osa_distance)
/* Not in the reference: the Indel similarity (STRSIM_INDEL of strsim_amd.h: 1 - (|a| + |b| - 2 LCS) / (|a| + |b|), rapidfuzz's
 * fuzz.ratio / 100), Float64 named after input 0 like the similarities above, and its integer distance |a| + |b| - 2 LCS (a
 * substitution costs 2), UInt32 with the optional max_distance input of the *_distance functions above. */
POLARS_PLUGIN_DECLARE(indel)
POLARS_PLUGIN_DECLARE(indel_distance)
/* Not in the reference: the partial ratio (STRSIM_PARTIAL_RATIO of strsim_amd.h: the best Indel similarity of the shorter string
 * against a window of the longer one, rapidfuzz's fuzz.partial_ratio / 100), Float64 named after input 0, through the same pipeline
 * as the similarities above; and the same with its alignment (strsim_partial_alignment_host): one Arrow struct chunk {score: Float64,
 * src_start, src_end, dest_start, dest_end: UInt32} named after input 0 -- src is input 0, dest input 1 (rapidfuzz's names), half-open
 * spans in Unicode scalar values.  Shape rule, literal broadcast and nulls (null in, null out) as above; no kwargs.  The alignment
 * call bypasses the small-call combiner. */
POLARS_PLUGIN_DECLARE(partial_ratio)
POLARS_PLUGIN_DECLARE(partial_ratio_alignment)
/* Not in the reference: token_sort_ratio and token_set_ratio (STRSIM_TOKEN_SORT_RATIO, STRSIM_TOKEN_SET_RATIO of strsim_amd.h:
 * rapidfuzz's fuzz.token_sort_ratio / 100 and fuzz.token_set_ratio / 100, tokens split at Python's str.isspace set), Float64 named
 * after input 0, through the same pipeline as the similarities above.  Shape rule, literal broadcast and nulls as above; no kwargs. */
POLARS_PLUGIN_DECLARE(token_sort_ratio)
POLARS_PLUGIN_DECLARE(token_set_ratio)
/* Not in the reference: token_ratio, partial_token_sort_ratio, partial_token_set_ratio, partial_token_ratio and wratio
 * (STRSIM_TOKEN_RATIO .. STRSIM_WRATIO of strsim_amd.h: rapidfuzz's fuzz.token_ratio, fuzz.partial_token_sort_ratio,
 * fuzz.partial_token_set_ratio, fuzz.partial_token_ratio and fuzz.WRatio, each / 100, without a processor), Float64 named after
 * input 0, through the same pipeline as the similarities above.  Shape rule, literal broadcast and nulls as above; no kwargs. */
POLARS_PLUGIN_DECLARE(token_ratio)
POLARS_PLUGIN_DECLARE(partial_token_sort_ratio)
POLARS_PLUGIN_DECLARE(partial_token_set_ratio)
POLARS_PLUGIN_DECLARE(partial_token_ratio)
POLARS_PLUGIN_DECLARE(wratio)

/* Best match (not in the reference): input 0 = the query column (N rows), input 1 = the candidate column (any number of rows; the
 * length rule of the functions above does not apply).  Output: N rows of an Arrow struct {index: UInt32, score: Float64} named after
 * input 0 -- the candidate with the highest score (ties to the lower index; the index is its row in input 1), as
 * strsim_best_match_host with k = 1.  Null where the query is null or there is no (non-null) candidate; null candidates are never
 * matched.  No kwargs. */
POLARS_PLUGIN_DECLARE(best_match_levenshtein)
POLARS_PLUGIN_DECLARE(best_match_jaro)
POLARS_PLUGIN_DECLARE(best_match_jaro_winkler)
POLARS_PLUGIN_DECLARE(best_match_jaccard)
POLARS_PLUGIN_DECLARE(best_match_sorensen_dice)

/* Nearest match by bounded edit distance (not in the reference): inputs 0 and 1 as best match (queries, candidates of any length),
 * an optional input 2 is max_distance, parsed as the *_distance functions parse it.  Output: N rows of an Arrow struct
 * {index: UInt32, distance: UInt32} named after input 0 -- the candidate with the smallest Levenshtein / OSA distance within
 * max_distance (ties to the lower index; the index is its row in input 1), as strsim_nearest_host with k = 1.  Null where the query
 * is null or no non-null candidate is within max_distance; null candidates are never matched. */
POLARS_PLUGIN_DECLARE(nearest_levenshtein)
POLARS_PLUGIN_DECLARE(nearest_osa)

/* Extract: the best candidate by ratio or token_sort_ratio with a score cutoff (not in the reference; rapidfuzz's
 * process.extractOne with fuzz.ratio / 100 or fuzz.token_sort_ratio / 100): inputs 0 and 1 as best match (queries, candidates of
 * any length), an optional input 2 is score_cutoff, one Float64 value (a null or absent input: no cutoff; NaN, more than one row or
 * another dtype is an error that names score_cutoff).  Output: N rows of an Arrow struct {index: UInt32, score: Float64} named after
 * input 0 -- the candidate with the highest score >= score_cutoff (ties to the lower index; the index is its row in input 1), as
 * strsim_extract_host with k = 1.  Null where the query is null or no non-null candidate reaches score_cutoff; null candidates are
 * never matched. */
POLARS_PLUGIN_DECLARE(extract_ratio)
POLARS_PLUGIN_DECLARE(extract_token_sort_ratio)

/* cdist: the scores of every query against every candidate (not in the reference; rapidfuzz's process.cdist with scores / 100, the
 * matrix of strsim_cdist_host row by row): inputs 0 and 1 as extract (queries, candidates of any length M), an optional input 2 is
 * score_cutoff, parsed as extract parses it; a score below it is 0.0.  Output: N rows of an Arrow LargeList<Float64> ("+L", child
 * "item") named after input 0 -- row i is the list of the M scores of query i, in the order of input 1.  A null query gives a null
 * list; a null candidate gives a null element (the child's validity) at its position in every list. */
POLARS_PLUGIN_DECLARE(cdist_levenshtein)
POLARS_PLUGIN_DECLARE(cdist_jaro)
POLARS_PLUGIN_DECLARE(cdist_jaro_winkler)
POLARS_PLUGIN_DECLARE(cdist_jaccard)
POLARS_PLUGIN_DECLARE(cdist_sorensen_dice)
POLARS_PLUGIN_DECLARE(cdist_ratio)
POLARS_PLUGIN_DECLARE(cdist_token_sort_ratio)

/* join: every candidate that scores at least score_cutoff (not in the reference; the pairs rapidfuzz's process.cdist leaves non-zero
 * under a score_cutoff, strsim_join_host): inputs 0 and 1 as extract (queries, candidates of any length), an optional input 2 is
 * score_cutoff, parsed as extract parses it (a null or absent input: every pair).  Output: N rows of an Arrow
 * LargeList<Struct{index: UInt32, score: Float64}> ("+L", child "item") named after input 0 -- row i is the list of the hits of query
 * i in ascending candidate index (its row in input 1), nothing truncated; a query without a hit gives an empty list.  A null query
 * gives a null list; null candidates are never matched. */
POLARS_PLUGIN_DECLARE(join_ratio)
POLARS_PLUGIN_DECLARE(join_token_sort_ratio)

/* match_join: the same by one of the five reference measures (strsim_match_join_host): every candidate whose score by the measure
 * is at least min_score.  Inputs, the optional input 2 (here min_score; it is parsed as join's score_cutoff and the messages about
 * it say score_cutoff), the null rules and the LargeList<Struct{index: UInt32, score: Float64}> result are join_ratio's. */
POLARS_PLUGIN_DECLARE(match_join_levenshtein)
POLARS_PLUGIN_DECLARE(match_join_jaro)
POLARS_PLUGIN_DECLARE(match_join_jaro_winkler)
POLARS_PLUGIN_DECLARE(match_join_jaccard)
POLARS_PLUGIN_DECLARE(match_join_sorensen_dice)

/* cluster: the duplicate groups of ONE column (not in the reference; strsim_cluster_host: the self-join of the column at
 * min_score, then the connected components of its hits).  Input 0 is a string series of any number of chunks, clustered as one
 * column; input 1 is the Float64 literal min_score (required: one non-null value, not NaN -- without it the call fails with
 * "cluster: expected 2 input series (the column and the Float64 literal min_score), got 1").  Output: N rows of UInt32 ("I") named
 * after input 0 -- row r holds the row of the first member of r's group.  A null row gives null and never joins anything.  Groups
 * chain: a ~ b and b ~ c put a and c together even where they do not match each other. */
POLARS_PLUGIN_DECLARE(cluster_ratio)
POLARS_PLUGIN_DECLARE(cluster_token_sort_ratio)
POLARS_PLUGIN_DECLARE(cluster_levenshtein)
POLARS_PLUGIN_DECLARE(cluster_jaro)
POLARS_PLUGIN_DECLARE(cluster_jaro_winkler)
POLARS_PLUGIN_DECLARE(cluster_jaccard)
POLARS_PLUGIN_DECLARE(cluster_sorensen_dice)

/* default_process (not in the reference; rapidfuzz's utils.default_process made context-free, strsim_default_process_host of
 * strsim_amd.h): ONE input, a string series in any of the three layouts; elementwise.  Output: N rows of Arrow Utf8 ("u": int32
 * offsets -- the transform's 32-bit offsets are the buffer as it is; a result beyond 2^31 - 1 bytes is an error) named after
 * input 0, one chunk, null where the input is null.  The field function declares "u".  The validity, offsets and values buffers
 * belong to the array's release callback. */
POLARS_PLUGIN_DECLARE(default_process)

/* Unrestricted Damerau-Levenshtein (not in the reference module; strsim::damerau_levenshtein of the crate, strsim_damerau_host and
 * strsim_damerau_distance_host of strsim_amd.h): the similarity, Float64 named after input 0 like the similarities above, and the
 * integer distance, UInt32 with the optional max_distance input 2 of the *_distance functions above.  Null where either input is
 * null.  These calls bypass the small-call combiner. */
POLARS_PLUGIN_DECLARE(damerau_levenshtein)
POLARS_PLUGIN_DECLARE(damerau_levenshtein_distance)

/* Hamming, prefix, postfix and LCSseq (not in the reference module; strsim_common_host, strsim_common_distance_host and
 * strsim_common_count_host of strsim_amd.h; rapidfuzz.distance.{Hamming, Prefix, Postfix, LCSseq}), three functions a kind: the
 * normalised similarity, Float64 named after input 0 like the similarities above; <kind>_distance, UInt32 with the optional
 * max_distance input 2 of the *_distance functions above (Hamming pads: the difference of the lengths counts); <kind>_similarity,
 * the count of common characters, UInt32, two inputs only.  Null where either input is null.  These calls bypass the small-call
 * combiner. */
POLARS_PLUGIN_DECLARE(hamming)
POLARS_PLUGIN_DECLARE(hamming_distance)
POLARS_PLUGIN_DECLARE(hamming_similarity)
POLARS_PLUGIN_DECLARE(prefix)
POLARS_PLUGIN_DECLARE(prefix_distance)
POLARS_PLUGIN_DECLARE(prefix_similarity)
POLARS_PLUGIN_DECLARE(postfix)
POLARS_PLUGIN_DECLARE(postfix_distance)
POLARS_PLUGIN_DECLARE(postfix_similarity)
POLARS_PLUGIN_DECLARE(lcs_seq)
POLARS_PLUGIN_DECLARE(lcs_seq_distance)
POLARS_PLUGIN_DECLARE(lcs_seq_similarity)

/* q-gram similarity (not in the reference; strsim_qgram_host of strsim_amd.h): Jaccard, Sorensen-Dice, overlap and cosine over the
 * q-grams of the two strings.  Inputs 0 and 1 as for the similarities (shape rule, literal broadcast, nulls); input 2 is q, a
 * length-1 non-null UInt32 series holding 1, 2 or 3 (required: without it the call fails with "q is missing: ..."); an optional
 * input 3 is the set flag, a length-1 non-null UInt32 series holding 0 (multisets of grams, the default) or 1 (sets).  Output: one
 * Float64 chunk named after input 0, null where either input is null.  These calls bypass the small-call combiner. */
POLARS_PLUGIN_DECLARE(qgram_jaccard)
POLARS_PLUGIN_DECLARE(qgram_sorensen_dice)
POLARS_PLUGIN_DECLARE(qgram_overlap)
POLARS_PLUGIN_DECLARE(qgram_cosine)

/* qgram_join: match_join by q-gram similarity (strsim_qgram_join_host): every candidate whose q-gram score of the kind is at least
 * min_score.  Inputs 0 and 1 are the queries and the candidates as for join_ratio; input 2 is q and input 3 the set flag, as for
 * qgram_jaccard (both required here); an optional input 4 is min_score (parsed as join's score_cutoff).  The null rules and the
 * LargeList<Struct{index: UInt32, score: Float64}> result are join_ratio's.
 * qgram_cluster: cluster by q-gram similarity (strsim_qgram_cluster_host).  Input 0 is the column, input 1 q, input 2 the set flag,
 * input 3 the Float64 literal min_score (required); the UInt32 result and the null rule are cluster_ratio's. */
POLARS_PLUGIN_DECLARE(qgram_join_jaccard)
POLARS_PLUGIN_DECLARE(qgram_join_sorensen_dice)
POLARS_PLUGIN_DECLARE(qgram_join_overlap)
POLARS_PLUGIN_DECLARE(qgram_join_cosine)
POLARS_PLUGIN_DECLARE(qgram_cluster_jaccard)
POLARS_PLUGIN_DECLARE(qgram_cluster_sorensen_dice)
POLARS_PLUGIN_DECLARE(qgram_cluster_overlap)
POLARS_PLUGIN_DECLARE(qgram_cluster_cosine)

/* distance_join: the join by integer edit distance (strsim_distance_join_host): every candidate within max_distance edits of the
 * query, by Levenshtein, OSA or the unrestricted Damerau-Levenshtein distance.  Inputs 0 and 1 are the queries and the candidates as
 * for join_ratio; an optional input 2 is max_distance, a length-1 UInt32 series (null or absent: every pair).  The null rules are
 * join_ratio's; the result is a LargeList<Struct{index: UInt32, distance: UInt32}>, the hits in ascending candidate index.
 * distance_cluster: cluster by edit distance (strsim_distance_cluster_host).  Input 0 is the column, input 1 the UInt32 literal
 * max_distance (required, not null); the UInt32 result and the null rule are cluster_ratio's. */
POLARS_PLUGIN_DECLARE(distance_join_levenshtein)
POLARS_PLUGIN_DECLARE(distance_join_osa)
POLARS_PLUGIN_DECLARE(distance_join_damerau_levenshtein)
POLARS_PLUGIN_DECLARE(distance_cluster_levenshtein)
POLARS_PLUGIN_DECLARE(distance_cluster_osa)
POLARS_PLUGIN_DECLARE(distance_cluster_damerau_levenshtein)

/* ---- diagnostics of this implementation (not part of the polars-ffi contract; the engine never calls them) ----
 * The plugin's staging -- pinned host memory and its device mirrors, per pipeline set -- is leased per call from one process-wide
 * pool under POLARS_STRSIM_STAGING_BUDGET_MB (csrc/plugin_pack.h: StagingPool; reference counterpart: the per-call scratch of
 * strsim.rs:78-84, :109-123).  out[0..7] = live pinned bytes, live device bytes, budget bytes (0 = none), pipeline sets, sets in use,
 * sets released so far, calls that had to wait for the budget, peak live bytes seen when a call returned. */
POLARS_PLUGIN_API void _polars_plugin_strsim_staging_stats(uint64_t out[8]);
/* Small calls of concurrent engine threads are combined into one launch when enough of them are in flight (csrc/plugin_pipeline.h:
 * Combiner; POLARS_STRSIM_COALESCE / _COALESCE_MIN_INFLIGHT / _COALESCE_ROWS).  out[0..3] = combined launches, the calls they
 * carried, the most calls in one launch, small calls that took the ordinary path. */
POLARS_PLUGIN_API void _polars_plugin_strsim_coalesce_stats(uint64_t out[4]);
/* Change the budget of a running process (tests; 0 = no budget).  Takes effect with the next call. */
POLARS_PLUGIN_API void _polars_plugin_strsim_staging_set_budget_mb(uint64_t megabytes);

#ifdef __cplusplus
}
#endif
#endif /* POLARS_PLUGIN_ABI_H */
