// plugin_process.h -- the default_process plugin function: one string series in, one string series out (the plugin's first
// string result).  Included by polars_plugin.cpp inside its anonymous namespace, after plugin_match.h.
//
// Input 0 is the string series, in any of the three layouts ("vu", "u", "U"), chunked or sliced.  It is packed whole (nulls as empty
// strings) and runs through strsim_default_process_host on a context leased from the staging pool.  The result is ONE Arrow Utf8
// ("u") chunk: validity, int32 offsets, values.  Utf8 and not LargeUtf8 because the transform's 32-bit offsets ARE the Arrow
// offsets buffer -- nothing is widened or copied -- and the engine casts either to its own string layout; the price is that a
// result of more than 2^31 - 1 bytes is refused (split the column).  The validity is the input's, rebuilt for the one chunk; the
// three buffers belong to the array's release callback.
#pragma once

struct StringArrayPriv {
    void *validity, *offsets, *values;
    const void *bufs[3];
};

void release_string_array(ArrowArray *a)
{
    if (!a || !a->release) return;
    StringArrayPriv *p = static_cast<StringArrayPriv *>(a->private_data);
    if (p) {
        free(p->validity);
        free(p->offsets);
        free(p->values);
        delete p;
    }
    a->release = nullptr;
}

// Hands the three buffers of a Utf8 array to `ret` as one chunk named `name`.  They are the caller's until this returns.
void export_string(const char *name, uint64_t n, uint8_t *validity, int64_t null_count, uint32_t *offsets, uint8_t *values, SeriesExport *ret)
{
    ArrowSchema *schema = static_cast<ArrowSchema *>(calloc(1, sizeof(ArrowSchema)));
    ArrowArray *arr = static_cast<ArrowArray *>(calloc(1, sizeof(ArrowArray)));
    ArrowArray **arrays = static_cast<ArrowArray **>(calloc(1, sizeof(ArrowArray *)));
    std::unique_ptr<StringArrayPriv> ap;
    std::unique_ptr<SeriesPriv> sp;
    try {
        if (!schema || !arr || !arrays) throw std::bad_alloc();
        ap.reset(new StringArrayPriv{validity, offsets, values, {validity, offsets, values}});
        sp.reset(new SeriesPriv{schema, arrays, 1});
        fill_named_schema(schema, "u", name); // (the last step that may throw)
    } catch (...) {
        free(schema); free(arr); free(arrays);
        throw;
    }
    arr->length = (int64_t)n;
    arr->null_count = null_count;
    arr->n_buffers = 3;
    arr->buffers = ap->bufs;
    arr->release = release_string_array;
    arr->private_data = ap.release();
    arrays[0] = arr;
    ret->field = schema;
    ret->arrays = arrays;
    ret->len = 1;
    ret->release = release_series;
    ret->private_data = sp.release();
}

void run_default_process(SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 1) fail("default_process: expected 1 input series, got " + std::to_string(n_inputs));
    Column c;
    describe(inputs[0], c);
    const uint64_t n = c.rows;
    if (range_bytes(c, 0, n) > 0xFFFFFFFFull) fail("default_process: a column of more than 4 GiB of string data");
    std::vector<uint32_t> off;
    std::vector<uint8_t> val;
    pack_column(c, false, off, val, nullptr);
    const uint64_t bytes = off[n], room = STRSIM_DEFAULT_PROCESS_CAPACITY(bytes);

    uint32_t *out_off = static_cast<uint32_t *>(alloc64((n + 1) * sizeof(uint32_t)));
    uint8_t *out_val = nullptr, *validity = nullptr;
    struct Cleanup {
        uint32_t *&o; uint8_t *&d; uint8_t *&v; bool armed = true;
        ~Cleanup() { if (armed) { free(o); free(d); free(v); } }
    } cleanup{out_off, out_val, validity};
    out_val = static_cast<uint8_t *>(alloc64(room));
    out_off[0] = 0u;
    if (n != 0) {
        PipeLease lease(2 * (bytes + 4 * (n + 1)) + room + 8 * (n + 1)); // the staged column, the new one, the work list
        if (strsim_default_process_host(leased_context(lease), off.data(), val.data(), n, out_off, out_val, room) != STRSIM_OK)
            fail(strsim_last_error_message());
        if (out_off[n] > 0x7FFFFFFFu) fail("default_process: the processed column holds more than 2^31 - 1 bytes; split the column");
    }
    int64_t null_count = 0;
    if (c.any_null && n != 0) {
        validity = static_cast<uint8_t *>(alloc64((n + 63) / 64 * 8));
        memset(validity, 0, (n + 63) / 64 * 8);
        for (uint64_t r = 0; r < n; ++r) {
            if (row_valid(c, r)) validity[r >> 3] |= (uint8_t)(1u << (r & 7));
            else ++null_count;
        }
    }
    export_string(c.name.c_str(), n, validity, null_count, out_off, out_val, ret);
    cleanup.armed = false;
}
