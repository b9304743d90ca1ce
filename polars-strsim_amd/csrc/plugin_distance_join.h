// plugin_distance_join.h -- the distance_join_<kind> and distance_cluster_<kind> plugin functions (kind: levenshtein, osa,
// damerau_levenshtein): the join and the duplicate groups by integer edit distance.  Included by polars_plugin.cpp inside its
// anonymous namespace, after plugin_cluster.h: they are run_join_values of plugin_join.h over strsim_distance_join_host and
// run_cluster_cut of plugin_cluster.h over strsim_distance_cluster_host, with the null handling and the messages of
// match_join_<measure> and cluster_<measure>.
//
// max_distance travels as the distance functions take it (plugin_match.h: uint32_literal): a length-1 UInt32 series behind the
// string inputs.
//   distance_join_<kind>     input 0 the queries, input 1 the candidates, an optional input 2 max_distance (null or absent: every
//                            pair) -> LargeList<Struct{index: UInt32, distance: UInt32}>
//   distance_cluster_<kind>  input 0 the column, input 1 max_distance (required, not null) -> UInt32
#pragma once

// the nullable LargeList<Struct{index, distance}> named `name`
void fill_list_distance_schema(ArrowSchema *s, const char *name) { fill_list_struct_schema_of(s, name, NEAREST_STRUCT); }

// Whether the length-1 series `s` holds a null (a series of another length is left to uint32_literal's messages).
bool literal_is_null(const SeriesExport &s)
{
    uint64_t rows = 0;
    const ArrowArray *one = nullptr;
    for (size_t i = 0; i < s.len; ++i) {
        const ArrowArray *a = s.arrays[i];
        if (!a || a->length == 0) continue;
        rows += (uint64_t)a->length;
        one = a;
    }
    if (rows != 1) return false;
    const uint8_t *valid = one->n_buffers > 0 ? static_cast<const uint8_t *>(one->buffers[0]) : nullptr;
    return one->null_count > 0 || (valid && !bit_at(valid, one->offset));
}

void run_distance_join(int kind, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2 && n_inputs != 3)
        fail("distance_join: expected 2 input series (queries, candidates) and an optional max_distance, got " + std::to_string(n_inputs));
    run_join_values<uint32_t>(
        [=](strsim_ctx_t *ctx, const uint32_t *qo, const uint8_t *qv, uint64_t n, const uint32_t *co, const uint8_t *cv, uint64_t m, uint32_t k,
            uint64_t capacity, uint64_t *indptr, uint32_t *index, uint32_t *dist, uint64_t *nnz) {
            return strsim_distance_join_host(ctx, kind, qo, qv, n, co, cv, m, k, 0u, capacity, indptr, index, dist, nnz);
        },
        [&]() -> uint32_t {
            if (n_inputs == 2 || literal_is_null(inputs[2])) return STRSIM_DISTANCE_UNBOUNDED;
            return uint32_literal(inputs[2], "max_distance");
        },
        NEAREST_STRUCT, inputs, n_inputs, ret);
}

void run_distance_cluster(int kind, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2)
        fail("distance_cluster: expected 2 input series (the column and the UInt32 literal max_distance), got " + std::to_string(n_inputs));
    run_cluster_cut(
        [=](strsim_ctx_t *ctx, const uint32_t *off, const uint8_t *val, uint64_t rows, uint32_t k, uint32_t *root, uint64_t *count) {
            return strsim_distance_cluster_host(ctx, kind, off, val, rows, k, root, nullptr, count, nullptr);
        },
        inputs, [&] { return uint32_literal(inputs[1], "max_distance"); }, ret);
}
