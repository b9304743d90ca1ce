// plugin_extract.h -- the extract_ratio / extract_token_sort_ratio plugin functions: the best candidate (k = 1) of every query row
// by ratio (Indel similarity) or token_sort_ratio, as an Arrow struct {index: UInt32, score: Float64}.  Included by
// polars_plugin.cpp inside its anonymous namespace, after plugin_nearest.h.
//
// Inputs as best_match_<measure> (plugin_match.h): input 0 the queries (N rows, the output has N rows), input 1 the candidates (any
// M; null candidates are dropped and the indices map back to rows of input 1); an optional input 2 is score_cutoff, one Float64
// value (null or absent: no cutoff).  The struct is null where the query is null or no non-null candidate reaches score_cutoff.
#pragma once

// score_cutoff from input 2 (-inf without one, or for a null)
double extract_cutoff(SeriesExport *inputs, size_t n_inputs)
{
    if (n_inputs == 2) return -__builtin_inf();
    const SeriesExport &s = inputs[2];
    if (!s.field || !s.field->format || strcmp(s.field->format, "g") != 0)
        fail(std::string("score_cutoff must be a Float64 series, got Arrow format '") + (s.field && s.field->format ? s.field->format : "") + "'");
    uint64_t rows = 0;
    const ArrowArray *one = nullptr;
    for (size_t i = 0; i < s.len; ++i) {
        const ArrowArray *a = s.arrays[i];
        if (!a || a->length == 0) continue;
        rows += (uint64_t)a->length;
        one = a;
    }
    if (rows != 1) fail("score_cutoff must be a single value, got " + std::to_string(rows) + " rows");
    const uint8_t *valid = one->n_buffers > 0 ? static_cast<const uint8_t *>(one->buffers[0]) : nullptr;
    if (one->null_count > 0 || (valid && !bit_at(valid, one->offset))) return -__builtin_inf();
    if (one->n_buffers < 2 || !one->buffers[1]) fail("score_cutoff: the Float64 series has no data buffer");
    const double v = static_cast<const double *>(one->buffers[1])[one->offset];
    if (v != v) fail("score_cutoff must not be NaN");
    return v;
}

void run_extract(int scorer, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2 && n_inputs != 3)
        fail("extract: expected 2 input series (queries, candidates) and an optional score_cutoff, got " + std::to_string(n_inputs));
    const SearchInputs in("extract", inputs, n_inputs, false);
    const double cutoff = extract_cutoff(inputs, n_inputs);
    const uint64_t n = in.q.rows;
    const Packed p(in.q, in.c, true);
    const uint64_t m = p.b_rows();
    StructOwned own(n, MATCH_STRUCT);
    if (n) {
        // staging and search workspace as nearest's (8-byte scores), and the normalised columns of token_sort_ratio on top
        const uint64_t lists = std::min<uint64_t>((uint64_t)1 << 24, n * 65535u) + n;
        PipeLease lease(2 * p.staged_bytes() + 16 * n + 84 * (n + m) + 12 * lists);
        if (strsim_extract_host(leased_context(lease), scorer, p.ao.data(), p.av.data(), n, p.bo.data(), p.bv.data(), m, 1, cutoff,
                                own.child<uint32_t>(0), own.child<double>(1)) != STRSIM_OK)
            fail(strsim_last_error_message());
    }
    const int64_t nulls = finish_search<double>(in.q, p.pos, n, own);
    export_struct(own, n, nulls, in.q.name.c_str(), MATCH_STRUCT, ret);
}
