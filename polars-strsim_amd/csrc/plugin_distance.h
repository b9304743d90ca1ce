// plugin_distance.h -- the levenshtein_distance / osa_distance / indel_distance plugin functions: bounded integer edit distances as one Arrow
// UInt32 ("I") chunk.  Included by polars_plugin.cpp inside its anonymous namespace, after plugin_match.h.
//
// Inputs 0 and 1 are the two string series, with the shape rule, literal broadcast, null handling and error messages of the
// similarity functions.  An optional input 2 carries max_distance: a length-1, non-null UInt32 series (Polars pickles keyword
// arguments; a literal series needs no parsing).  The strings are packed with the best-match packers and the distances run through
// strsim_distance_host on a context leased from the staging pool.  These calls bypass the small-call combiner.
#pragma once

// max_distance from input 2 (STRSIM_DISTANCE_UNBOUNDED without one)
uint32_t distance_cutoff(SeriesExport *inputs, size_t n_inputs)
{
    if (n_inputs == 2) return STRSIM_DISTANCE_UNBOUNDED;
    const SeriesExport &s = inputs[2];
    if (!s.field || !s.field->format || strcmp(s.field->format, "I") != 0)
        fail(std::string("max_distance must be a UInt32 series, got Arrow format '") + (s.field && s.field->format ? s.field->format : "") + "'");
    uint64_t rows = 0;
    const ArrowArray *one = nullptr;
    for (size_t i = 0; i < s.len; ++i) {
        const ArrowArray *a = s.arrays[i];
        if (!a || a->length == 0) continue;
        rows += (uint64_t)a->length;
        one = a;
    }
    if (rows != 1) fail("max_distance must be a single value, got " + std::to_string(rows) + " rows");
    const uint8_t *valid = one->n_buffers > 0 ? static_cast<const uint8_t *>(one->buffers[0]) : nullptr;
    if (one->null_count > 0 || (valid && !bit_at(valid, one->offset))) fail("max_distance must not be null");
    if (one->n_buffers < 2 || !one->buffers[1]) fail("max_distance: the UInt32 series has no data buffer");
    return static_cast<const uint32_t *>(one->buffers[1])[one->offset];
}

void run_distance(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2 && n_inputs != 3)
        fail("expected 2 input series and an optional max_distance, got " + std::to_string(n_inputs));
    Column col[2];
    describe(inputs[0], col[0]);
    describe(inputs[1], col[1]);
    const Column &a = col[0], &b = col[1];
    if (a.rows != b.rows && a.rows != 1 && b.rows != 1) // strsim.rs:48-52
        fail("Inputs must have the same length, or one of them must be a Utf8 literal.");
    const uint32_t k = distance_cutoff(inputs, n_inputs);
    const bool lit[2] = {a.rows == 1 && b.rows != 1, b.rows == 1};
    const uint64_t n = lit[0] ? b.rows : a.rows;
    const bool all_null = (lit[0] && !row_valid(a, 0)) || (lit[1] && !row_valid(b, 0));

    uint32_t *out = static_cast<uint32_t *>(alloc64(n * sizeof(uint32_t)));
    uint8_t *validity = nullptr;
    struct Cleanup {
        uint32_t *&o; uint8_t *&v; bool armed = true;
        ~Cleanup() { if (armed) { free(o); free(v); } }
    } cleanup{out, validity};
    if (n != 0 && !all_null) {
        std::vector<uint32_t> ao, bo;
        std::vector<uint8_t> av, bv;
        pack_column(a, false, ao, av, nullptr);
        pack_column(b, false, bo, bv, nullptr);
        // the lease is for its context: staged strings, offsets and outputs, the work list and the wave tier's scratch
        const uint64_t need = 2 * (av.size() + bv.size() + 4 * (a.rows + b.rows + 2)) + 8 * n;
        PipeLease lease(need);
        strsim_ctx_t *ctx = lease.set->at(0).open(plugin_devices()[0]);
        if (strsim_distance_host(ctx, measure, ao.data(), av.data(), a.rows, bo.data(), bv.data(), b.rows, k, out, n) != STRSIM_OK)
            fail(strsim_last_error_message());
    }
    int64_t null_count = 0;
    if ((all_null || a.any_null || b.any_null) && n != 0) {
        validity = static_cast<uint8_t *>(alloc64((n + 63) / 64 * 8));
        const uint64_t *vw = reinterpret_cast<const uint64_t *>(validity);
        null_count = build_validity(col, lit, n, all_null, 1, reinterpret_cast<uint64_t *>(validity), nullptr);
        for (uint64_t r = 0; r < n; ++r) // (values under nulls: 0, never observable)
            if (!((vw[r >> 6] >> (r & 63)) & 1u)) out[r] = 0u;
    }

    ArrowSchema *schema = static_cast<ArrowSchema *>(calloc(1, sizeof(ArrowSchema)));
    ArrowArray *arr = static_cast<ArrowArray *>(calloc(1, sizeof(ArrowArray)));
    ArrowArray **arrays = static_cast<ArrowArray **>(calloc(1, sizeof(ArrowArray *)));
    if (!schema || !arr || !arrays) { free(schema); free(arr); free(arrays); throw std::bad_alloc(); }
    try {
        fill_named_schema(schema, "I", a.name.c_str());
    } catch (...) {
        free(schema); free(arr); free(arrays);
        throw;
    }
    ArrayPriv *ap = new ArrayPriv{out, validity, {validity, out}, false};
    arr->length = (int64_t)n;
    arr->null_count = null_count;
    arr->offset = 0;
    arr->n_buffers = 2;
    arr->n_children = 0;
    arr->buffers = ap->bufs;
    arr->release = release_f64_array; // (frees the data and validity buffers: nothing in it is specific to f64)
    arr->private_data = ap;
    cleanup.armed = false;
    SeriesPriv *sp = new SeriesPriv{schema, arrays, 1};
    sp->arrays[0] = arr;
    ret->field = schema;
    ret->arrays = sp->arrays;
    ret->len = 1;
    ret->release = release_series;
    ret->private_data = sp;
}

void distance_entry(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    InputGuard guard{inputs, n_inputs};
    try {
        run_distance(measure, inputs, n_inputs, ret);
    } catch (const PluginError &e) {
        g_plugin_error = e.msg;
    } catch (const std::bad_alloc &) {
        g_plugin_error = "out of host memory";
    } catch (const std::exception &e) {
        g_plugin_error = std::string("unexpected failure: ") + e.what();
    } catch (...) {
        g_plugin_error = "unexpected failure";
    }
}

// output_type=UInt32, named after the first input
void distance_field_entry(ArrowSchema *input_fields, size_t n_fields, ArrowSchema *ret)
{
    const char *name = (n_fields > 0 && input_fields && input_fields[0].name) ? input_fields[0].name : "";
    try {
        fill_named_schema(ret, "I", name);
    } catch (...) {
        memset(ret, 0, sizeof *ret);
        g_plugin_error = "out of host memory";
    }
}
