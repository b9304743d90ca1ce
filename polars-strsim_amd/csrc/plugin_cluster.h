// plugin_cluster.h -- the cluster_<measure> plugin functions: the duplicate groups of ONE string column as a UInt32 column of the
// same length named after it -- row r holds the row of the first member of r's group (its root), so that group_by on the result
// groups the duplicates.  Included by polars_plugin.cpp inside its anonymous namespace, after plugin_join.h.
//
// Input 0 is the column (any number of chunks: it is clustered as one column), input 1 the Float64 literal min_score (required: one
// non-null value, not NaN).  Null rows are dropped before the call and the roots map back to rows of input 0: a null row gives
// null and never joins anything.  The call is strsim_cluster_host: the pairs of the self-join stay on the device.
#pragma once

const char *const CLUSTER_NO_LITERAL = "cluster: expected 2 input series (the column and the Float64 literal min_score), got ";

// min_score from input 1
double cluster_min_score(const SeriesExport &s)
{
    if (!s.field || !s.field->format || strcmp(s.field->format, "g") != 0)
        fail(std::string("min_score must be a Float64 series, got Arrow format '") + (s.field && s.field->format ? s.field->format : "") + "'");
    uint64_t rows = 0;
    const ArrowArray *one = nullptr;
    for (size_t i = 0; i < s.len; ++i) {
        const ArrowArray *a = s.arrays[i];
        if (!a || a->length == 0) continue;
        rows += (uint64_t)a->length;
        one = a;
    }
    if (rows != 1) fail("min_score must be a single value, got " + std::to_string(rows) + " rows");
    const uint8_t *valid = one->n_buffers > 0 ? static_cast<const uint8_t *>(one->buffers[0]) : nullptr;
    if (one->null_count > 0 || (valid && !bit_at(valid, one->offset))) fail("min_score must not be null (it would put every row in one group)");
    if (one->n_buffers < 2 || !one->buffers[1]) fail("min_score: the Float64 series has no data buffer");
    const double v = static_cast<const double *>(one->buffers[1])[one->offset];
    if (v != v) fail("min_score must not be NaN");
    return v;
}

// Frees what has not been handed over.
struct ClusterOwned {
    void *root = nullptr, *valid = nullptr;
    ~ClusterOwned() { free(root); free(valid); }
};

// cluster_host(ctx, offsets, values, rows, cutoff, out_root, &count): the family's host entry point with its measure bound.  The
// column is input 0; cutoff() parses the family's cutoff (behind the column's own check, as the messages are ordered).
template <class ClusterHost, class Cutoff>
void run_cluster_cut(ClusterHost cluster_host, SeriesExport *inputs, Cutoff cutoff, SeriesExport *ret)
{
    Column col;
    describe(inputs[0], col);
    if (col.rows > 0xFFFFFFFEull) fail("cluster: more than 2^32 - 2 rows");
    const auto min_score = cutoff();
    const uint64_t n = col.rows;
    std::vector<uint32_t> off, pos;
    std::vector<uint8_t> val;
    pack_column(col, true, off, val, &pos);
    const uint64_t m = off.size() - 1; // the rows that are not null
    ClusterOwned own;
    own.root = alloc64(n * sizeof(uint32_t));
    if (col.any_null) own.valid = alloc64((n + 63) / 64 * 8);
    uint32_t *const root = static_cast<uint32_t *>(own.root);
    uint8_t *const valid = static_cast<uint8_t *>(own.valid);
    if (m) {
        // staging, the join's workspace (as run_join), its CSR at the first capacity, parent, the flags' scan and the labels
        PipeLease lease(4 * (val.size() + 4 * off.size()) + 16 * m + 2 * 84 * m + 4 * 65 * m + 16 * 8 * m + 12 * (4 * m + 1024) + 24 * m);
        uint64_t count = 0;
        if (cluster_host(leased_context(lease), off.data(), val.data(), m, min_score, root, &count) != STRSIM_OK) fail(strsim_last_error_message());
    }
    // packed row x -> row pos[x] of the column, back to front: pos[x] >= x, so no root is overwritten before it is read
    int64_t nulls = 0;
    if (valid) {
        memset(valid, 0, (n + 63) / 64 * 8);
        for (uint64_t x = m; x-- > 0;) root[pos[x]] = pos[root[x]];
        for (uint64_t x = 0; x < m; ++x) valid[pos[x] >> 3] |= (uint8_t)(1u << (pos[x] & 7));
        for (uint64_t r = 0; r < n; ++r)
            if (!(valid[r >> 3] >> (r & 7) & 1)) { root[r] = 0; ++nulls; }
    }
    export_primitive("I", col.name.c_str(), n, own.root, valid, nulls, false, ret);
    own.root = own.valid = nullptr;
}

// The families that cut by an f64 score: min_score is the Float64 literal `min_score_input`.
template <class ClusterHost>
void run_cluster_call(ClusterHost cluster_host, SeriesExport *inputs, const SeriesExport &min_score_input, SeriesExport *ret)
{
    run_cluster_cut(cluster_host, inputs, [&] { return cluster_min_score(min_score_input); }, ret);
}

void run_cluster(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2) fail(CLUSTER_NO_LITERAL + std::to_string(n_inputs));
    run_cluster_call(
        [=](strsim_ctx_t *ctx, const uint32_t *off, const uint8_t *val, uint64_t rows, double min_score, uint32_t *root, uint64_t *count) {
            return strsim_cluster_host(ctx, measure, off, val, rows, min_score, root, nullptr, count, nullptr);
        },
        inputs, inputs[1], ret);
}
