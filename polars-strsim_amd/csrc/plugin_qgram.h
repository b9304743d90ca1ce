// plugin_qgram.h -- the qgram_jaccard / qgram_sorensen_dice / qgram_overlap / qgram_cosine plugin functions: q-gram similarity as one
// Arrow Float64 ("g") chunk named after input 0.  Included by polars_plugin.cpp inside its anonymous namespace, after
// plugin_distance.h.
//
// Inputs 0 and 1 are the two string series, with the shape rule, literal broadcast, null handling and error messages of the
// similarity functions.  Input 2 carries q and the optional input 3 the set flag (0: multisets, 1: sets), each a length-1, non-null
// UInt32 series as max_distance is for the distance functions.  The strings are packed with the best-match packers and the scores
// run through strsim_qgram_host on a context leased from the staging pool.  These calls bypass the small-call combiner.
#pragma once

void run_qgram(int kind, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs < 3) fail("q is missing: expected 2 input series, q and an optional set flag, got " + std::to_string(n_inputs) + " inputs");
    if (n_inputs > 4) fail("expected 2 input series, q and an optional set flag, got " + std::to_string(n_inputs) + " inputs");
    const Elementwise e(inputs);
    const uint32_t q = uint32_literal(inputs[2], "q");
    if (q < 1u || q > 3u) fail("q=" + std::to_string(q) + " is outside 1..3");
    const uint32_t set = n_inputs == 4 ? uint32_literal(inputs[3], "the set flag") : 0u;
    if (set > 1u) fail("the set flag must be 0 or 1, got " + std::to_string(set));
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
        if (strsim_qgram_host(leased_context(lease), kind, q, set ? STRSIM_QGRAM_SET : 0u, p.ao.data(), p.av.data(), p.a_rows(), p.bo.data(),
                              p.bv.data(), p.b_rows(), out, n) != STRSIM_OK)
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
