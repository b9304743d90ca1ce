// plugin_distance.h -- the levenshtein_distance / osa_distance / indel_distance plugin functions: bounded integer edit distances as one Arrow
// UInt32 ("I") chunk.  Included by polars_plugin.cpp inside its anonymous namespace, after plugin_match.h.
//
// Inputs 0 and 1 are the two string series, with the shape rule, literal broadcast, null handling and error messages of the
// similarity functions.  An optional input 2 carries max_distance: a length-1, non-null UInt32 series (Polars pickles keyword
// arguments; a literal series needs no parsing).  The strings are packed with the best-match packers and the distances run through
// strsim_distance_host on a context leased from the staging pool.  These calls bypass the small-call combiner.
#pragma once

void run_distance(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
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
        if (strsim_distance_host(leased_context(lease), measure, p.ao.data(), p.av.data(), p.a_rows(), p.bo.data(), p.bv.data(), p.b_rows(), k,
                                 out, n) != STRSIM_OK)
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
