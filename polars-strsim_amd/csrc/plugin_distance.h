// plugin_distance.h -- the levenshtein_distance / osa_distance / indel_distance / damerau_levenshtein_distance plugin functions:
// bounded integer edit distances as one Arrow UInt32 ("I") chunk; and damerau_levenshtein, the similarity that has no measure id, as
// one Float64 ("g") chunk.  Included by polars_plugin.cpp inside its anonymous namespace, after plugin_match.h.
//
// Inputs 0 and 1 are the two string series, with the shape rule, literal broadcast, null handling and error messages of the
// similarity functions.  An optional input 2 carries max_distance: a length-1, non-null UInt32 series (Polars pickles keyword
// arguments; a literal series needs no parsing).  The strings are packed with the best-match packers and the distances run through
// strsim_distance_host (strsim_damerau_distance_host) on a context leased from the staging pool.  These calls bypass the small-call
// combiner.
#pragma once

// host(ctx, a_off, a_val, a_rows, b_off, b_val, b_rows, max_distance, out, n): the C ABI call that fills the distances
template <class Host>
void run_distance_by(Host &&host, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2 && n_inputs != 3)
        fail("expected 2 input series and an optional max_distance, got " + std::to_string(n_inputs));
    const Elementwise e(inputs);
    const uint32_t k = distance_cutoff(inputs, n_inputs);
    const uint64_t n = e.n;

    uint32_t *out = static_cast<uint32_t *>(alloc64(n * sizeof(uint32_t)));
    uint8_t *validity = nullptr;
    struct Cleanup {
        uint32_t *&o; uint8_t *&v; bool armed = true;
        ~Cleanup() { if (armed) { free(o); free(v); } }
    } cleanup{out, validity};
    if (n != 0 && !e.all_null) {
        const Packed p(e.col[0], e.col[1], false);
        PipeLease lease(p.staged_bytes() + 8 * n); // + the outputs and the work list
        if (host(leased_context(lease), p.ao.data(), p.av.data(), p.a_rows(), p.bo.data(), p.bv.data(), p.b_rows(), k, out, n) != STRSIM_OK)
            fail(strsim_last_error_message());
    }
    int64_t null_count = 0;
    if (e.any_null() && n != 0) {
        validity = static_cast<uint8_t *>(alloc64((n + 63) / 64 * 8));
        const uint64_t *vw = reinterpret_cast<const uint64_t *>(validity);
        null_count = build_validity(e.col, e.lit, n, e.all_null, 1, reinterpret_cast<uint64_t *>(validity), nullptr);
        for (uint64_t r = 0; r < n; ++r) // (values under nulls: 0, never observable)
            if (!((vw[r >> 6] >> (r & 63)) & 1u)) out[r] = 0u;
    }
    export_primitive("I", e.col[0].name.c_str(), n, out, validity, null_count, false, ret);
    cleanup.armed = false;
}

void run_distance(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    run_distance_by(
        [measure](strsim_ctx_t *c, const uint32_t *ao, const uint8_t *av, uint64_t ar, const uint32_t *bo, const uint8_t *bv, uint64_t br,
                  uint32_t k, uint32_t *out, uint64_t n) { return strsim_distance_host(c, measure, ao, av, ar, bo, bv, br, k, out, n); },
        inputs, n_inputs, ret);
}

void run_damerau_distance(SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    run_distance_by(strsim_damerau_distance_host, inputs, n_inputs, ret);
}

// A similarity that has no measure id, one Float64 chunk named after input 0.
// host(ctx, a_off, a_val, a_rows, b_off, b_val, b_rows, out, n): the C ABI call that fills the similarities
template <class Host>
void run_similarity_by(Host &&host, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2) fail("expected 2 input series, got " + std::to_string(n_inputs));
    const Elementwise e(inputs);
    const uint64_t n = e.n;

    double *out = static_cast<double *>(alloc64(n * sizeof(double)));
    uint8_t *validity = nullptr;
    struct Cleanup {
        double *&o; uint8_t *&v; bool armed = true;
        ~Cleanup() { if (armed) { free(o); free(v); } }
    } cleanup{out, validity};
    if (n != 0 && !e.all_null) {
        const Packed p(e.col[0], e.col[1], false);
        PipeLease lease(p.staged_bytes() + 12 * n); // + the outputs and the work list
        if (host(leased_context(lease), p.ao.data(), p.av.data(), p.a_rows(), p.bo.data(), p.bv.data(), p.b_rows(), out, n) != STRSIM_OK)
            fail(strsim_last_error_message());
    } else {
        for (uint64_t r = 0; r < n; ++r) out[r] = 0.0;
    }
    int64_t null_count = 0;
    if (e.any_null() && n != 0) {
        validity = static_cast<uint8_t *>(alloc64((n + 63) / 64 * 8));
        // (values under nulls: 0, never observable)
        null_count = build_validity(e.col, e.lit, n, e.all_null, 1, reinterpret_cast<uint64_t *>(validity), out);
    }
    export_primitive("g", e.col[0].name.c_str(), n, out, validity, null_count, false, ret);
    cleanup.armed = false;
}

// damerau_levenshtein: the similarity through strsim_damerau_host
void run_damerau(SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    run_similarity_by(strsim_damerau_host, inputs, n_inputs, ret);
}
