// plugin_partial.h -- the partial_ratio_alignment plugin function: the partial ratio of every row with the window that won, as one
// Arrow struct chunk {score: Float64, src_start, src_end, dest_start, dest_end: UInt32} named after input 0 (src = input 0, dest =
// input 1; half-open spans in Unicode scalar values).  Included by polars_plugin.cpp inside its anonymous namespace, after
// plugin_distance.h.
//
// Shape rule, literal broadcast, null handling (null in, null out) and error messages of the similarity functions.  The strings
// are packed with the best-match packers and run through strsim_partial_alignment_host on a context leased from the staging pool;
// the struct is best match's (plugin_match.h: export_struct; every child owns its copy of the validity).  Bypasses the small-call
// combiner.
#pragma once

void run_partial_alignment(SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2) fail("expected 2 input series, got " + std::to_string(n_inputs));
    const Elementwise e(inputs);
    const uint64_t n = e.n;

    StructOwned own(n, PARTIAL_STRUCT);
    double *const score = own.child<double>(0);
    std::vector<uint32_t> span(n * 4 + 4, 0u);
    if (n != 0 && !e.all_null) {
        const Packed p(e.col[0], e.col[1], false);
        PipeLease lease(p.staged_bytes() + 28 * n); // + the outputs and the work list
        if (strsim_partial_alignment_host(leased_context(lease), p.ao.data(), p.av.data(), p.a_rows(), p.bo.data(), p.bv.data(), p.b_rows(), score,
                                          span.data(), n) != STRSIM_OK)
            fail(strsim_last_error_message());
    } else {
        for (uint64_t r = 0; r < n; ++r) score[r] = 0.0;
    }
    uint64_t *const vw = static_cast<uint64_t *>(own.valid);
    int64_t nulls = 0;
    if (e.any_null() && n != 0) nulls = build_validity(e.col, e.lit, n, e.all_null, 1, vw, nullptr);
    else memset(own.valid, 0xFF, (n + 63) / 64 * 8);
    for (uint64_t r = 0; r < n; ++r) { // (values under nulls: 0, never observable)
        const bool ok = (vw[r >> 6] >> (r & 63)) & 1u;
        if (!ok) score[r] = 0.0;
        for (int k = 0; k < 4; ++k) own.child<uint32_t>(1 + k)[r] = ok ? span[4 * r + k] : 0u;
    }
    export_struct(own, n, nulls, e.col[0].name.c_str(), PARTIAL_STRUCT, ret);
}
