// plugin_nearest.h -- the nearest_levenshtein / nearest_osa plugin functions: the nearest candidate (k = 1) of every query row by
// bounded edit distance, as an Arrow struct {index: UInt32, distance: UInt32}.  Included by polars_plugin.cpp inside its
// anonymous namespace, after plugin_distance.h.
//
// Inputs as best_match_<measure> (plugin_match.h): input 0 the queries (N rows, the output has N rows), input 1 the candidates (any
// M; null candidates are dropped and the indices map back to rows of input 1); an optional input 2 is max_distance, parsed as the
// distance functions parse it.  The struct is null where the query is null or no non-null candidate is within max_distance.
#pragma once

void run_nearest(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2 && n_inputs != 3)
        fail("nearest: expected 2 input series (queries, candidates) and an optional max_distance, got " + std::to_string(n_inputs));
    Column q, c;
    describe(inputs[0], q);
    describe(inputs[1], c);
    const uint32_t k = distance_cutoff(inputs, n_inputs);
    if (q.rows > 0xFFFFFFFFull) fail("nearest: more than 2^32 - 1 queries");
    if (c.rows > 0xFFFFFFFEull) fail("nearest: more than 2^32 - 2 candidates");
    const uint64_t n = q.rows;
    std::vector<uint32_t> qo, co, pos;
    std::vector<uint8_t> qv, cv;
    pack_column(q, false, qo, qv, nullptr);
    pack_column(c, true, co, cv, &pos);
    const uint64_t m = pos.size();

    const size_t vbytes = (n + 63) / 64 * 8;
    MatchOwned own(n, 4);
    uint32_t *const idx = static_cast<uint32_t *>(own.buf[0]);
    uint32_t *const dist = static_cast<uint32_t *>(own.buf[1]);
    uint8_t *const valid = static_cast<uint8_t *>(own.buf[2]);
    if (n) {
        // the lease is for its context: staging and search workspace as best match's, with 4-byte outputs, the length-ordered
        // candidates and the fallback's distance batches on top
        const uint64_t lists = std::min<uint64_t>((uint64_t)1 << 24, n * 65535u) + n;
        const uint64_t need = 2 * (qv.size() + cv.size() + 4 * (n + m + 2)) + 16 * n + 84 * (n + m) + 12 * lists;
        PipeLease lease(need);
        strsim_ctx_t *ctx = lease.set->at(0).open(plugin_devices()[0]);
        if (strsim_nearest_host(ctx, measure, qo.data(), qv.data(), n, co.data(), cv.data(), m, 1, k, idx, dist) != STRSIM_OK)
            fail(strsim_last_error_message());
    }
    int64_t nulls = 0;
    memset(valid, 0, vbytes);
    for (uint64_t r = 0; r < n; ++r) {
        const bool ok = idx[r] != 0xFFFFFFFFu && row_valid(q, r);
        if (ok) { valid[r >> 3] |= (uint8_t)(1u << (r & 7)); idx[r] = pos[idx[r]]; }
        else { ++nulls; idx[r] = 0; dist[r] = 0; }
    }
    export_match_struct(own, n, nulls, q.name.c_str(), "distance", "I", ret);
}

void nearest_entry(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    InputGuard guard{inputs, n_inputs};
    try {
        run_nearest(measure, inputs, n_inputs, ret);
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

// {index: UInt32, distance: UInt32}, named after the first input
void nearest_field_entry(ArrowSchema *input_fields, size_t n_fields, ArrowSchema *ret)
{
    const char *name = (n_fields > 0 && input_fields && input_fields[0].name) ? input_fields[0].name : "";
    try {
        fill_match_schema(ret, name, "distance", "I");
    } catch (...) { // (no exception crosses the ABI: an unreleasable, empty schema is left behind)
        memset(ret, 0, sizeof *ret);
        g_plugin_error = "out of host memory";
    }
}
