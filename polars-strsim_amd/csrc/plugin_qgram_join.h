// plugin_qgram_join.h -- the qgram_join_<kind> and qgram_cluster_<kind> plugin functions (kind: jaccard, sorensen_dice, overlap,
// cosine): the threshold join and the duplicate groups by q-gram similarity.  Included by polars_plugin.cpp inside its anonymous
// namespace, after plugin_cluster.h: they are run_join_call of plugin_join.h over strsim_qgram_join_host and run_cluster_call of
// plugin_cluster.h over strsim_qgram_cluster_host, with the outputs, the null handling and the messages of match_join_<measure> and
// cluster_<measure>.
//
// q and the set flag (0: multisets, 1: sets) travel as the qgram_<kind> functions take them (plugin_qgram.h): each a length-1,
// non-null UInt32 series, behind the string inputs.
//   qgram_join_<kind>     input 0 the queries, input 1 the candidates, input 2 q, input 3 the set flag, an optional input 4
//                         min_score (Float64; null or absent: every pair)
//   qgram_cluster_<kind>  input 0 the column, input 1 q, input 2 the set flag, input 3 the Float64 literal min_score (required)
#pragma once

// q from `q_input` and STRSIM_QGRAM_SET or 0 from `set_input`, with run_qgram's messages
void qgram_mode(const SeriesExport &q_input, const SeriesExport &set_input, uint32_t *q, uint32_t *qflags)
{
    *q = uint32_literal(q_input, "q");
    if (*q < 1u || *q > 3u) fail("q=" + std::to_string(*q) + " is outside 1..3");
    const uint32_t set = uint32_literal(set_input, "the set flag");
    if (set > 1u) fail("the set flag must be 0 or 1, got " + std::to_string(set));
    *qflags = set ? STRSIM_QGRAM_SET : 0u;
}

void run_qgram_join(int kind, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 4 && n_inputs != 5)
        fail("qgram_join: expected 2 input series (queries, candidates), q, the set flag and an optional min_score, got " + std::to_string(n_inputs));
    uint32_t q, qflags;
    qgram_mode(inputs[2], inputs[3], &q, &qflags);
    // run_join_call reads the queries, the candidates and the optional cutoff: the same series, q and the flag left out
    SeriesExport view[3] = {inputs[0], inputs[1], inputs[n_inputs == 5 ? 4 : 0]};
    run_join_call(
        [=](strsim_ctx_t *ctx, const uint32_t *qo, const uint8_t *qv, uint64_t n, const uint32_t *co, const uint8_t *cv, uint64_t m, double cutoff,
            uint64_t capacity, uint64_t *indptr, uint32_t *index, double *score, uint64_t *nnz) {
            return strsim_qgram_join_host(ctx, kind, q, qflags, qo, qv, n, co, cv, m, cutoff, 0u, capacity, indptr, index, score, nnz);
        },
        view, n_inputs - 2, ret);
}

void run_qgram_cluster(int kind, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 4)
        fail("qgram_cluster: expected 4 input series (the column, q, the set flag and the Float64 literal min_score), got " + std::to_string(n_inputs));
    uint32_t q, qflags;
    qgram_mode(inputs[1], inputs[2], &q, &qflags);
    run_cluster_call(
        [=](strsim_ctx_t *ctx, const uint32_t *off, const uint8_t *val, uint64_t rows, double min_score, uint32_t *root, uint64_t *count) {
            return strsim_qgram_cluster_host(ctx, kind, q, qflags, off, val, rows, min_score, root, nullptr, count, nullptr);
        },
        inputs, inputs[3], ret);
}
