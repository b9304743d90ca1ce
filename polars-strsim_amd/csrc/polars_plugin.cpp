// polars_plugin.cpp -- the Polars expression-plugin ABI (include/polars_plugin_abi.h) on top of the
// gfx950 kernels: the C++ counterpart of the reference's macro glue (reference src/expressions/mod.rs:8-31)
// and of `strsim::parallel_apply` (reference src/expressions/strsim.rs:41-107).
//
// What happens per call (one Polars expression evaluation):
//   1. both input Series (any chunking; Arrow "vu" string views as Polars >= 0.20 sends them, or "u"/"U"
//      offset layouts) are described in place; shape rule and literal broadcast exactly as strsim.rs:48-52,61-66;
//   2. rows are cut into slices of 2 M rows; each slice is packed by helper threads (none when the engine says it
//      is already parallel, strsim.rs:53) into the device layout -- uint32 offsets + packed UTF-8 values -- in pinned
//      staging memory;
//   3. a two-slot software pipeline overlaps packing slice k+1 with H2D + kernels of slice k (strsim_pairs_device);
//   4. the f64 column comes back as one Arrow "g" chunk whose validity is the AND of the inputs'
//      validities (null in -> null out, README.md:69-70); values under null slots are computed like the
//      reference's arity helpers do and are never observable.
// Nothing here computes similarities on the CPU; without a GPU the call fails with the plugin's error message.
//
// Documented divergences from the reference: a length-1 literal on the LEFT is broadcast over
// every row of the right column in both engine modes (the reference's rayon branch splits by a.len() == 1,
// strsim.rs:73, and silently returns one row); a NULL literal yields an all-null column instead of the
// reference's `unwrap()` panic (strsim.rs:62,65,87,90).
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <emmintrin.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include "polars_plugin_abi.h"
#include "strsim_amd.h"
#include "strsim_internal.h"

namespace {

thread_local std::string g_plugin_error;

struct PluginError {
    std::string msg;
};

[[noreturn]] void fail(const std::string &m) { throw PluginError{m}; }

#include "plugin_arrow.h"
#include "plugin_pack.h"
#include "plugin_pipeline.h"

// ---- pieces every plugin function is made of --------------------------------------------------------

// A plugin call: the callee owns the inputs whatever happens, and no exception crosses the ABI -- a failure leaves `ret` empty
// and its message in g_plugin_error.
template <class Fn> void guarded(SeriesExport *inputs, size_t n_inputs, Fn fn)
{
    InputGuard guard{inputs, n_inputs};
    try {
        fn();
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

// A planning-time field: fill(ret, name of input 0).  (No exception crosses the ABI: an unreleasable, empty schema is left behind.)
template <class Fill> void field_named_after_input0(ArrowSchema *input_fields, size_t n_fields, ArrowSchema *ret, Fill fill)
{
    const char *name = (n_fields > 0 && input_fields && input_fields[0].name) ? input_fields[0].name : "";
    try {
        fill(ret, name);
    } catch (...) {
        memset(ret, 0, sizeof *ret);
        g_plugin_error = "out of host memory";
    }
}

void fill_named_schema(ArrowSchema *s, const char *format, const char *name)
{
    fill_f64_schema(s, name);
    s->format = format;
}

// The two columns of an elementwise function: shape rule and literal broadcast exactly as strsim.rs:48-52,61-66.
struct Elementwise {
    Column col[2];
    bool lit[2];
    uint64_t n;
    bool all_null; // a NULL literal: the reference unwrap()s and panics (strsim.rs:62,65,87,90); here every row is null
    explicit Elementwise(SeriesExport *inputs)
    {
        describe(inputs[0], col[0]);
        describe(inputs[1], col[1]);
        const Column &a = col[0], &b = col[1];
        if (a.rows != b.rows && a.rows != 1 && b.rows != 1)
            fail("Inputs must have the same length, or one of them must be a Utf8 literal.");
        lit[0] = a.rows == 1 && b.rows != 1;
        lit[1] = b.rows == 1;
        n = lit[0] ? b.rows : a.rows;
        all_null = (lit[0] && !row_valid(a, 0)) || (lit[1] && !row_valid(b, 0));
    }
    bool any_null() const { return all_null || col[0].any_null || col[1].any_null; }
};

// Hands `data` (n values of Arrow format `format`; pinned: from pinned_pool()) and `validity` (or nullptr) to `ret` as one
// chunk named `name`.  They are the caller's until this returns.
void export_primitive(const char *format, const char *name, uint64_t n, void *data, uint8_t *validity, int64_t null_count, bool pinned,
                      SeriesExport *ret)
{
    ArrowSchema *schema = static_cast<ArrowSchema *>(calloc(1, sizeof(ArrowSchema)));
    ArrowArray *arr = static_cast<ArrowArray *>(calloc(1, sizeof(ArrowArray)));
    ArrowArray **arrays = static_cast<ArrowArray **>(calloc(1, sizeof(ArrowArray *)));
    std::unique_ptr<ArrayPriv> ap;
    std::unique_ptr<SeriesPriv> sp;
    try {
        if (!schema || !arr || !arrays) throw std::bad_alloc();
        ap.reset(new ArrayPriv{data, validity, {validity, data}, pinned});
        sp.reset(new SeriesPriv{schema, arrays, 1});
        fill_named_schema(schema, format, name); // (the last step that may throw)
    } catch (...) {
        free(schema); free(arr); free(arrays);
        throw;
    }
    arr->length = (int64_t)n;
    arr->null_count = null_count;
    arr->n_buffers = 2;
    arr->buffers = ap->bufs;
    arr->release = release_f64_array; // (frees the data and validity buffers: nothing in it is specific to f64)
    arr->private_data = ap.release();
    arrays[0] = arr;
    ret->field = schema;
    ret->arrays = arrays;
    ret->len = 1;
    ret->release = release_series;
    ret->private_data = sp.release();
}
#include "plugin_match.h"
#include "plugin_distance.h"
#include "plugin_common.h"
#include "plugin_qgram.h"
#include "plugin_partial.h"
#include "plugin_nearest.h"
#include "plugin_extract.h"
#include "plugin_cdist.h"
#include "plugin_join.h"
#include "plugin_cluster.h"
#include "plugin_qgram_join.h"
#include "plugin_distance_join.h"
#include "plugin_process.h"

void run(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret, bool engine_parallel)
{
    PhaseTimer tm;
    const auto t_begin = std::chrono::steady_clock::now();
    if (n_inputs != 2) fail("expected 2 input series, got " + std::to_string(n_inputs));
    const Elementwise e(inputs);
    const Column(&col)[2] = e.col;
    const bool(&lit)[2] = e.lit;
    const uint64_t n = e.n;
    const bool all_null = e.all_null;

    double *out = static_cast<double *>(pinned_pool().acquire(n * sizeof(double))); // large columns (see PinnedPool)
    const bool out_pinned = out != nullptr;
    if (!out) out = static_cast<double *>(alloc64(n * sizeof(double)));
    uint8_t *validity = nullptr;
    int64_t null_count = 0;
    struct Cleanup {
        double *&o; bool pinned; uint8_t *&v; bool armed = true;
        ~Cleanup() { if (armed) { if (pinned) pinned_pool().release(o); else free(o); free(v); } }
    } cleanup{out, out_pinned, validity};

    const PackGrant grant(engine_parallel, n); // (helper threads borrowed for an engine-parallel call go back when it returns)
    const unsigned T = grant.threads;
    std::vector<PipeTimes> ptimes;
    std::vector<int> devs = plugin_devices();
    if (n != 0 && !all_null) {
        const bool direct_call = n <= direct_rows();
        const uint64_t D = std::max<uint64_t>(1, std::min<uint64_t>(devs.size(), n / min_rows_per_device()));
        devs.resize((size_t)D);
        bool combined = false;
        if (direct_call) {
            // a small call: when enough of them are in flight at once they share a launch (plugin_pipeline.h: Combiner)
            const SmallCallGuard in_flight;
            const CoalesceKnobs &ck = coalesce_knobs();
            if (ck.on && D == 1 && !lit[0] && !lit[1] && n <= ck.rows && in_flight.before + 1 >= ck.min_inflight)
                combined = combiner().run(measure, col, n, out, devs[0]);
            if (!combined) {
                combiner().direct_.fetch_add(1, std::memory_order_relaxed);
                run_rows(measure, col, lit, n, out, out_pinned, T, direct_call, engine_parallel, devs, tm, ptimes);
            }
        } else {
            run_rows(measure, col, lit, n, out, out_pinned, T, direct_call, engine_parallel, devs, tm, ptimes);
        }
    }

    // output validity = AND of the input validities (broadcast for a literal; a null literal is the all_null case)
    if (e.any_null() && n != 0) {
        validity = static_cast<uint8_t *>(alloc64((n + 63) / 64 * 8));
        null_count = build_validity(col, lit, n, all_null, T, reinterpret_cast<uint64_t *>(validity), out);
    }
    export_primitive("g", col[0].name.c_str(), n, out, validity, null_count, out_pinned, ret); // one "g" chunk
    cleanup.armed = false;
    if (tm.on) {
        double launch = 0, wait = 0, d2h = 0;
        for (const PipeTimes &p : ptimes) { launch += p.t_launch; wait += p.t_wait; d2h += p.t_d2h; }
        fprintf(stderr, "[polars_strsim] rows=%llu total=%.2f ms: pack=%.2f launch=%.2f wait=%.2f d2h=%.2f copy=%.2f (threads %u, pipelines %zu)\n",
                (unsigned long long)n,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(), tm.t_pack,
                launch, wait, d2h, tm.t_copy, T, ptimes.size());
        for (size_t d = 0; d < ptimes.size(); ++d)
            fprintf(stderr, "[polars_strsim]   pipeline %zu (device %d): %u slices, launch=%.2f wait=%.2f d2h=%.2f ms\n", d, devs[d],
                    ptimes[d].slices, ptimes[d].t_launch, ptimes[d].t_wait, ptimes[d].t_d2h);
    }
}

// output_type=Float64 (mod.rs:8,13,18,23,28): a Float64 field carrying the first input's name
void field_entry(ArrowSchema *input_fields, size_t n_fields, ArrowSchema *ret)
{
    const char *name = (n_fields > 0 && input_fields && input_fields[0].name) ? input_fields[0].name : "";
    fill_f64_schema(ret, name);
}

} // namespace

extern "C" {

uint32_t _polars_plugin_get_version(void) { return (POLARS_PLUGIN_VERSION_MAJOR << 16) | POLARS_PLUGIN_VERSION_MINOR; }

const char *_polars_plugin_get_last_error_message(void) { return g_plugin_error.c_str(); }

void _polars_plugin_strsim_staging_stats(uint64_t out[8]) { if (out) staging_pool().stats(out); }
void _polars_plugin_strsim_staging_set_budget_mb(uint64_t megabytes) { staging_pool().set_budget(megabytes << 20); }
void _polars_plugin_strsim_coalesce_stats(uint64_t out[4]) { if (out) combiner().stats(out); }

// One exported function and its planning-time field: `call` runs under guarded(), `field` fills return_value.
#define POLARS_PLUGIN_EXPORT(name, call, field)                                                                  \
    void _polars_plugin_##name(SeriesExport *inputs, size_t n_inputs, const uint8_t *, size_t,                   \
                               SeriesExport *return_value, CallerContext *cc)                                    \
    {                                                                                                            \
        guarded(inputs, n_inputs, [&] { call; });                                                                \
    }                                                                                                            \
    void _polars_plugin_field_##name(ArrowSchema *input_fields, size_t n_fields, ArrowSchema *return_value)      \
    {                                                                                                            \
        field;                                                                                                   \
    }
#define STRUCT_FIELD(shape) \
    field_named_after_input0(input_fields, n_fields, return_value, [](ArrowSchema *s, const char *n) { fill_struct_schema(s, n, shape); })
#define POLARS_PLUGIN_DEFINE(name, id) \
    POLARS_PLUGIN_EXPORT(name, run(id, inputs, n_inputs, return_value, cc && (cc->bitflags & 1u)), field_entry(input_fields, n_fields, return_value))
#define POLARS_PLUGIN_DEFINE_DISTANCE(name, id)                                                \
    POLARS_PLUGIN_EXPORT(name##_distance, run_distance(id, inputs, n_inputs, return_value), \
                         field_named_after_input0(input_fields, n_fields, return_value, [](ArrowSchema *s, const char *n) { fill_named_schema(s, "I", n); }))
#define POLARS_PLUGIN_DEFINE_COMMON(name, kind)                                                                                   \
    POLARS_PLUGIN_EXPORT(name, run_common(kind, inputs, n_inputs, return_value), field_entry(input_fields, n_fields, return_value)) \
    POLARS_PLUGIN_EXPORT(name##_distance, run_common_distance(kind, inputs, n_inputs, return_value),                             \
                         field_named_after_input0(input_fields, n_fields, return_value, [](ArrowSchema *s, const char *n) { fill_named_schema(s, "I", n); })) \
    POLARS_PLUGIN_EXPORT(name##_similarity, run_common_count(kind, inputs, n_inputs, return_value),                              \
                         field_named_after_input0(input_fields, n_fields, return_value, [](ArrowSchema *s, const char *n) { fill_named_schema(s, "I", n); }))
#define POLARS_PLUGIN_DEFINE_QGRAM(name, kind) \
    POLARS_PLUGIN_EXPORT(qgram_##name, run_qgram(kind, inputs, n_inputs, return_value), field_entry(input_fields, n_fields, return_value))
#define POLARS_PLUGIN_DEFINE_NEAREST(name, id) \
    POLARS_PLUGIN_EXPORT(nearest_##name, run_nearest(id, inputs, n_inputs, return_value), STRUCT_FIELD(NEAREST_STRUCT))
#define POLARS_PLUGIN_DEFINE_EXTRACT(name, id) \
    POLARS_PLUGIN_EXPORT(extract_##name, run_extract(id, inputs, n_inputs, return_value), STRUCT_FIELD(MATCH_STRUCT))
#define POLARS_PLUGIN_DEFINE_CDIST(name, id)                                      \
    POLARS_PLUGIN_EXPORT(cdist_##name, run_cdist(id, inputs, n_inputs, return_value), \
                         field_named_after_input0(input_fields, n_fields, return_value, fill_list_f64_schema))
#define POLARS_PLUGIN_DEFINE_JOIN(name, id)                                     \
    POLARS_PLUGIN_EXPORT(join_##name, run_join(strsim_join_host, id, inputs, n_inputs, return_value), \
                         field_named_after_input0(input_fields, n_fields, return_value, fill_list_struct_schema))
#define POLARS_PLUGIN_DEFINE_MATCH_JOIN(name, id)                                                             \
    POLARS_PLUGIN_EXPORT(match_join_##name, run_join(strsim_match_join_host, id, inputs, n_inputs, return_value), \
                         field_named_after_input0(input_fields, n_fields, return_value, fill_list_struct_schema))
#define POLARS_PLUGIN_DEFINE_CLUSTER(name, id)                                        \
    POLARS_PLUGIN_EXPORT(cluster_##name, run_cluster(id, inputs, n_inputs, return_value), \
                         field_named_after_input0(input_fields, n_fields, return_value, [](ArrowSchema *s, const char *n) { fill_named_schema(s, "I", n); }))
#define POLARS_PLUGIN_DEFINE_QGRAM_JOIN(name, kind)                                                    \
    POLARS_PLUGIN_EXPORT(qgram_join_##name, run_qgram_join(kind, inputs, n_inputs, return_value),      \
                         field_named_after_input0(input_fields, n_fields, return_value, fill_list_struct_schema)) \
    POLARS_PLUGIN_EXPORT(qgram_cluster_##name, run_qgram_cluster(kind, inputs, n_inputs, return_value), \
                         field_named_after_input0(input_fields, n_fields, return_value, [](ArrowSchema *s, const char *n) { fill_named_schema(s, "I", n); }))
#define POLARS_PLUGIN_DEFINE_DISTANCE_JOIN(name, kind)                                                       \
    POLARS_PLUGIN_EXPORT(distance_join_##name, run_distance_join(kind, inputs, n_inputs, return_value),      \
                         field_named_after_input0(input_fields, n_fields, return_value, fill_list_distance_schema)) \
    POLARS_PLUGIN_EXPORT(distance_cluster_##name, run_distance_cluster(kind, inputs, n_inputs, return_value), \
                         field_named_after_input0(input_fields, n_fields, return_value, [](ArrowSchema *s, const char *n) { fill_named_schema(s, "I", n); }))
#define POLARS_PLUGIN_DEFINE_MATCH(name, id) \
    POLARS_PLUGIN_EXPORT(best_match_##name, run_best_match(id, inputs, n_inputs, return_value), STRUCT_FIELD(MATCH_STRUCT))

#ifdef STRSIM_TEST_HOOKS
// Test hooks (no GPU needed), compiled only into tests/cpu_harness/libplugin_testhooks.so (make testhooks) -- the product library
// does not export them.
// (1) the host-side packing of rows [r0, r1) of one Series with `threads` helper threads into caller-provided buffers -- the exact
// describe / range_bytes / pack_range code the plugin entry points use.  Owns and releases the input like a plugin call.
// Returns 0, or -1 with the message in _polars_plugin_get_last_error_message().
POLARS_PLUGIN_API int _strsim_test_pack_series(SeriesExport *series, uint64_t r0, uint64_t r1, uint32_t *off_out,
                                               uint8_t *val_out, uint64_t val_cap, uint64_t *rows_out, uint64_t *bytes_out,
                                               uint8_t *valid_out, unsigned threads)
{
    InputGuard guard{series, 1};
    try {
        Column c;
        describe(*series, c);
        if (rows_out) *rows_out = c.rows;
        if (r1 > c.rows) r1 = c.rows;
        if (r0 > r1) r0 = r1;
        const uint64_t rows = r1 - r0;
        unsigned T = threads ? threads : 1;
        if (T > rows) T = rows ? (unsigned)rows : 1;
        std::vector<uint64_t> part(T + 1, 0);
        auto lo = [&](unsigned t) { return r0 + rows * t / T; };
        fork_join(T, [&](unsigned t) { part[t + 1] = range_bytes(c, lo(t), lo(t + 1)); });
        for (unsigned t = 0; t < T; ++t) part[t + 1] += part[t];
        if (bytes_out) *bytes_out = part[T];
        if (part[T] + 16 > val_cap) fail("test buffer too small");
        off_out[0] = 0;
        fork_join(T, [&](unsigned t) { pack_range(c, lo(t), lo(t + 1), off_out + (lo(t) - r0), part[t], part[t + 1], val_out); });
        if (valid_out)
            for (uint64_t r = r0; r < r1; ++r) valid_out[r - r0] = row_valid(c, r) ? 1 : 0;
        return 0;
    } catch (const PluginError &e) {
        g_plugin_error = e.msg;
    } catch (...) {
        g_plugin_error = "unexpected failure";
    }
    return -1;
}

// (1b) the ONE-PASS packer on one view Series used for both columns of a slice: rows [r0, r1) on `threads` threads with a budget of
// bpr256 / 256 bytes per row.  Returns 1 and fills val_out (the segments CLOSED UP the way the device does: seg_dst order),
// len_out (one byte per row) and *bytes_out when the pass succeeds, 0 when it reports "overflow / long string" (the plugin then
// packs two-pass), -1 on error.
POLARS_PLUGIN_API int _strsim_test_pack_onepass(SeriesExport *series, uint64_t r0, uint64_t r1, uint64_t bpr256, unsigned threads,
                                                uint8_t *val_out, uint64_t val_cap, uint8_t *len_out, uint64_t *bytes_out, int *nseg_out)
{
    InputGuard guard{series, 1};
    try {
        Column col[2];
        describe(*series, col[0]);
        describe(*series, col[1]);
        if (col[0].layout != L_VIEW) fail("one-pass packing is for view columns");
        if (r1 > col[0].rows) r1 = col[0].rows;
        if (r0 > r1) r0 = r1;
        Slot sl; // (plain memory stands in for the pinned staging: generous enough that reserve() never allocates -- no GPU here)
        const uint64_t cap = (((r1 - r0) * bpr256) >> 8) + (r1 - r0) + 64 * 4096 + 65536;
        struct Free {
            Slot &s;
            ~Free() { for (int i = 0; i < 2; ++i) { free(s.h_val[i].p); free(s.h_len[i].p); s.h_val[i].p = s.h_len[i].p = nullptr; s.h_val[i].cap = s.h_len[i].cap = 0; } }
        } fr{sl};
        for (int i = 0; i < 2; ++i) {
            sl.h_val[i].p = malloc(cap); sl.h_val[i].cap = cap;
            sl.h_len[i].p = malloc(r1 - r0 + 64); sl.h_len[i].cap = r1 - r0 + 64;
        }
        uint64_t b[2] = {bpr256, bpr256};
        if (!pack_slice_onepass(col, r0, r1, sl, b, threads ? threads : 1)) return 0;
        if (sl.bytes[0] > val_cap) fail("test buffer too small");
        for (int k = 0; k < sl.nseg[0]; ++k)
            memcpy(val_out + sl.seg_dst[0][k], static_cast<const uint8_t *>(sl.h_val[0].p) + sl.seg_src[0][k], sl.seg_bytes[0][k]);
        memcpy(len_out, sl.h_len[0].p, r1 - r0);
        if (bytes_out) *bytes_out = sl.bytes[0];
        if (nseg_out) *nseg_out = sl.nseg[0];
        // both "columns" are the same series: their segments must agree
        if (sl.bytes[1] != sl.bytes[0] || sl.nseg[1] != sl.nseg[0]) fail("the two columns of the slice disagree");
        return 1;
    } catch (const PluginError &e) {
        g_plugin_error = e.msg;
    } catch (...) {
        g_plugin_error = "unexpected failure";
    }
    return -1;
}

// (1c) the VIEW-NATIVE form of one view Series used for both columns of a slice (pack_slice_views): rows [r0, r1) on `threads`
// threads; lbpr256: the long bytes per row (x 256) to size the segments by, ~0: size them exactly.  Fills views_out (16 bytes per
// row) and long_out (the segments as they lie, *span_out bytes) and *bytes_out (the packed size).  Returns 0 / -1.
POLARS_PLUGIN_API int _strsim_test_pack_views(SeriesExport *series, uint64_t r0, uint64_t r1, uint64_t lbpr256, unsigned threads,
                                              uint8_t *views_out, uint8_t *long_out, uint64_t long_cap, uint64_t *span_out, uint64_t *bytes_out)
{
    InputGuard guard{series, 1};
    try {
        Column col[2];
        describe(*series, col[0]);
        describe(*series, col[1]);
        if (col[0].layout != L_VIEW) fail("view-native packing is for view columns");
        if (r1 > col[0].rows) r1 = col[0].rows;
        if (r0 > r1) r0 = r1;
        Slot sl; // (plain memory stands in for the pinned staging: generous enough that reserve() never allocates -- no GPU here)
        struct Free {
            Slot &s;
            ~Free() { for (int i = 0; i < 2; ++i) { free(s.h_views[i].p); free(s.h_long[i].p); s.h_views[i].p = s.h_long[i].p = nullptr; s.h_views[i].cap = s.h_long[i].cap = 0; } }
        } fr{sl};
        const uint64_t lcap = range_bytes(col[0], r0, r1) + (r1 - r0) + 64 * 4096 + 65536 + (((r1 - r0) * (lbpr256 == ~0ull ? 0 : lbpr256)) >> 7);
        for (int i = 0; i < 2; ++i) {
            sl.h_views[i].p = malloc((r1 - r0) * 16 + 128); sl.h_views[i].cap = (r1 - r0) * 16 + 128;
            sl.h_long[i].p = malloc(lcap); sl.h_long[i].cap = lcap;
        }
        uint64_t l[2] = {lbpr256, lbpr256};
        if (!pack_slice_views(col, r0, r1, sl, l, threads ? threads : 1)) fail("the slice exceeds the per-slice byte limit");
        if (sl.long_span[0] > long_cap) fail("test buffer too small");
        memcpy(views_out, sl.h_views[0].p, (r1 - r0) * 16);
        memcpy(long_out, sl.h_long[0].p, sl.long_span[0]);
        if (span_out) *span_out = sl.long_span[0];
        if (bytes_out) *bytes_out = sl.bytes[0];
        if (sl.bytes[1] != sl.bytes[0] || memcmp(sl.h_views[0].p, sl.h_views[1].p, (r1 - r0) * 16) != 0) fail("the two columns of the slice disagree");
        return 0;
    } catch (const PluginError &e) {
        g_plugin_error = e.msg;
    } catch (...) {
        g_plugin_error = "unexpected failure";
    }
    return -1;
}

// (2) the output validity of a call over two Series (a one-row side is the literal), as the plugin builds it: words[(n + 63) / 64]
// and the null count; vals (optional, n doubles): the slots under nulls are zeroed.  Returns 0 / -1 like (1).
POLARS_PLUGIN_API int _strsim_test_validity(SeriesExport *two_series, uint64_t *words, int64_t *null_count, double *vals,
                                            uint64_t *rows_out, unsigned threads)
{
    InputGuard guard{two_series, 2};
    try {
        Column col[2];
        describe(two_series[0], col[0]);
        describe(two_series[1], col[1]);
        if (col[0].rows != col[1].rows && col[0].rows != 1 && col[1].rows != 1) fail("shape");
        const bool lit[2] = {col[0].rows == 1 && col[1].rows != 1, col[1].rows == 1};
        const uint64_t n = lit[0] ? col[1].rows : col[0].rows;
        if (rows_out) *rows_out = n;
        const bool all_null = (lit[0] && !row_valid(col[0], 0)) || (lit[1] && !row_valid(col[1], 0));
        *null_count = n ? build_validity(col, lit, n, all_null, threads ? threads : 1, words, vals) : 0;
        return 0;
    } catch (const PluginError &e) {
        g_plugin_error = e.msg;
    } catch (...) {
        g_plugin_error = "unexpected failure";
    }
    return -1;
}

// (3) the packing threads of `n_calls` engine-parallel calls of `rows` rows each that are ALL in flight together, entered one after
// the other (the staggered arrival of an engine's threads): threads_out[i] = what call i packs on.  *helpers_out = helper threads
// lent out while all of them run; the return value = the same count after all have returned (0).
POLARS_PLUGIN_API int _strsim_test_pack_grants(int engine_parallel, int n_calls, uint64_t rows, unsigned *threads_out, int *helpers_out)
{
    {
        std::vector<std::unique_ptr<PackGrant>> g;
        for (int i = 0; i < n_calls; ++i) {
            g.emplace_back(new PackGrant(engine_parallel != 0, rows));
            threads_out[i] = g.back()->threads;
        }
        *helpers_out = g_helpers_out.load();
    }
    return g_helpers_out.load();
}

// (4) the staging pool under `budget_bytes`: one call's lease of a pipeline set (`need` = its estimate), `grow` bytes of staging
// reserved in it (host memory in this build), held for `hold_us`, given back.  Called from many threads at once by the driver.
// stats8 (optional): _polars_plugin_strsim_staging_stats' eight counters after the call.
POLARS_PLUGIN_API int _strsim_test_staging_lease(uint64_t budget_bytes, uint64_t need, uint64_t grow, unsigned hold_us, uint64_t *stats8)
{
    try {
        staging_pool().set_budget(budget_bytes);
        {
            PipeLease lease(need);
            Pipe &P = lease.set->at(0);
            P.slot[(need >> 3) % 3].h_val[0].reserve(grow);
            memset(P.slot[(need >> 3) % 3].h_val[0].p, 0x5A, grow);
            if (hold_us) std::this_thread::sleep_for(std::chrono::microseconds(hold_us));
        }
        if (stats8) staging_pool().stats(stats8);
        return 0;
    } catch (const PluginError &e) {
        g_plugin_error = e.msg;
    } catch (...) {
        g_plugin_error = "unexpected failure";
    }
    return -1;
}

// (5) one small call through the combiner (plugin_pipeline.h), with a CPU stand-in for the combined launch: out[i] = 4096 * (bytes of
// row i of a) + (bytes of row i of b) + (first byte of a's row) / 256.  Owns and releases the two inputs like a plugin call.  Returns 1 when
// the call was combined, 0 when it was not eligible, -1 on failure.
static void test_combined_launch(const uint32_t *oa, const uint8_t *va, const uint32_t *ob, const uint8_t *, uint64_t rows, double *out)
{
    for (uint64_t i = 0; i < rows; ++i) {
        const uint32_t la = oa[i + 1] - oa[i], lb = ob[i + 1] - ob[i];
        out[i] = 4096.0 * la + lb + (la ? va[oa[i]] / 256.0 : 0.0);
    }
}
POLARS_PLUGIN_API int _strsim_test_combine(SeriesExport *two_series, int measure, double *out, uint64_t *rows_out)
{
    InputGuard guard{two_series, 2};
    try {
        Column col[2];
        describe(two_series[0], col[0]);
        describe(two_series[1], col[1]);
        if (col[0].rows != col[1].rows) fail("shape");
        if (rows_out) *rows_out = col[0].rows;
        static const bool stand_in = (combiner().test_launch = test_combined_launch, true); // (once: every caller thread comes through here)
        (void)stand_in;
        const SmallCallGuard in_flight;
        return col[0].rows && combiner().run(measure, col, col[0].rows, out, 0) ? 1 : 0;
    } catch (const PluginError &e) {
        g_plugin_error = e.msg;
    } catch (...) {
        g_plugin_error = "unexpected failure";
    }
    return -1;
}

// (6) a struct result of `n` synthetic rows (every third row null) through export_struct, released the way a consumer may: whole
// (move_child < 0), or with child `move_child` moved out first (Arrow C data interface: copied, its release cleared in the struct)
// and released after the struct is gone.  sum_out: the moved child's first 4-byte values, read after the struct's release.
POLARS_PLUGIN_API int _strsim_test_export_struct(uint64_t n, int move_child, uint64_t *sum_out)
{
    try {
        const StructShape &shape = PARTIAL_STRUCT;
        StructOwned own(n, shape);
        int64_t nulls = 0;
        memset(own.valid, 0, (n + 63) / 64 * 8);
        for (uint64_t r = 0; r < n; ++r) {
            if (r % 3 == 2) ++nulls; else static_cast<uint8_t *>(own.valid)[r >> 3] |= (uint8_t)(1u << (r & 7));
            own.child<double>(0)[r] = (double)r;
            for (int i = 1; i < shape.n; ++i) own.child<uint32_t>(i)[r] = (uint32_t)(r + (uint64_t)i);
        }
        SeriesExport ret{};
        export_struct(own, n, nulls, "synthetic", shape, &ret);
        ArrowArray arr = *ret.arrays[0]; // (the importer takes the arrays by bitwise copy, release_series frees the boxes)
        ArrowArray moved{};
        if (move_child >= 0) { moved = *arr.children[move_child]; arr.children[move_child]->release = nullptr; }
        const bool ok = arr.length == (int64_t)n && arr.null_count == nulls && arr.n_children == shape.n;
        arr.release(&arr);
        ret.release(&ret);
        uint64_t sum = 0;
        if (move_child >= 0) {
            for (uint64_t r = 0; r < n; ++r) sum += static_cast<const uint32_t *>(moved.buffers[1])[r];
            if (nulls && !moved.buffers[0]) fail("the moved child lost its validity");
            moved.release(&moved);
        }
        if (sum_out) *sum_out = sum;
        if (!ok) fail("struct header");
        return 0;
    } catch (const PluginError &e) {
        g_plugin_error = e.msg;
    } catch (...) {
        g_plugin_error = "unexpected failure";
    }
    return -1;
}
#endif // STRSIM_TEST_HOOKS

POLARS_PLUGIN_DEFINE(levenshtein, STRSIM_LEVENSHTEIN)
POLARS_PLUGIN_DEFINE(jaro, STRSIM_JARO)
POLARS_PLUGIN_DEFINE(jaro_winkler, STRSIM_JARO_WINKLER)
POLARS_PLUGIN_DEFINE(jaccard, STRSIM_JACCARD)
POLARS_PLUGIN_DEFINE(sorensen_dice, STRSIM_SORENSEN_DICE)
POLARS_PLUGIN_DEFINE(osa, STRSIM_OSA)
POLARS_PLUGIN_DEFINE(indel, STRSIM_INDEL)
POLARS_PLUGIN_DEFINE(partial_ratio, STRSIM_PARTIAL_RATIO)
POLARS_PLUGIN_DEFINE(token_sort_ratio, STRSIM_TOKEN_SORT_RATIO)
POLARS_PLUGIN_DEFINE(token_set_ratio, STRSIM_TOKEN_SET_RATIO)
POLARS_PLUGIN_DEFINE(token_ratio, STRSIM_TOKEN_RATIO)
POLARS_PLUGIN_DEFINE(partial_token_sort_ratio, STRSIM_PARTIAL_TOKEN_SORT_RATIO)
POLARS_PLUGIN_DEFINE(partial_token_set_ratio, STRSIM_PARTIAL_TOKEN_SET_RATIO)
POLARS_PLUGIN_DEFINE(partial_token_ratio, STRSIM_PARTIAL_TOKEN_RATIO)
POLARS_PLUGIN_DEFINE(wratio, STRSIM_WRATIO)
POLARS_PLUGIN_EXPORT(partial_ratio_alignment, run_partial_alignment(inputs, n_inputs, return_value), STRUCT_FIELD(PARTIAL_STRUCT))
POLARS_PLUGIN_DEFINE_DISTANCE(levenshtein, STRSIM_LEVENSHTEIN)
POLARS_PLUGIN_DEFINE_DISTANCE(osa, STRSIM_OSA)
POLARS_PLUGIN_DEFINE_DISTANCE(indel, STRSIM_INDEL)
POLARS_PLUGIN_EXPORT(damerau_levenshtein, run_damerau(inputs, n_inputs, return_value), field_entry(input_fields, n_fields, return_value))
POLARS_PLUGIN_EXPORT(damerau_levenshtein_distance, run_damerau_distance(inputs, n_inputs, return_value),
                     field_named_after_input0(input_fields, n_fields, return_value, [](ArrowSchema *s, const char *n) { fill_named_schema(s, "I", n); }))
POLARS_PLUGIN_DEFINE_COMMON(hamming, STRSIM_COMMON_HAMMING)
POLARS_PLUGIN_DEFINE_COMMON(prefix, STRSIM_COMMON_PREFIX)
POLARS_PLUGIN_DEFINE_COMMON(postfix, STRSIM_COMMON_POSTFIX)
POLARS_PLUGIN_DEFINE_COMMON(lcs_seq, STRSIM_COMMON_LCSSEQ)
POLARS_PLUGIN_DEFINE_QGRAM(jaccard, STRSIM_QGRAM_JACCARD)
POLARS_PLUGIN_DEFINE_QGRAM(sorensen_dice, STRSIM_QGRAM_SORENSEN_DICE)
POLARS_PLUGIN_DEFINE_QGRAM(overlap, STRSIM_QGRAM_OVERLAP)
POLARS_PLUGIN_DEFINE_QGRAM(cosine, STRSIM_QGRAM_COSINE)
POLARS_PLUGIN_DEFINE_NEAREST(levenshtein, STRSIM_LEVENSHTEIN)
POLARS_PLUGIN_DEFINE_NEAREST(osa, STRSIM_OSA)
POLARS_PLUGIN_DEFINE_EXTRACT(ratio, STRSIM_INDEL)
POLARS_PLUGIN_DEFINE_EXTRACT(token_sort_ratio, STRSIM_TOKEN_SORT_RATIO)
POLARS_PLUGIN_DEFINE_CDIST(levenshtein, STRSIM_LEVENSHTEIN)
POLARS_PLUGIN_DEFINE_CDIST(jaro, STRSIM_JARO)
POLARS_PLUGIN_DEFINE_CDIST(jaro_winkler, STRSIM_JARO_WINKLER)
POLARS_PLUGIN_DEFINE_CDIST(jaccard, STRSIM_JACCARD)
POLARS_PLUGIN_DEFINE_CDIST(sorensen_dice, STRSIM_SORENSEN_DICE)
POLARS_PLUGIN_DEFINE_CDIST(ratio, STRSIM_INDEL)
POLARS_PLUGIN_DEFINE_CDIST(token_sort_ratio, STRSIM_TOKEN_SORT_RATIO)
POLARS_PLUGIN_DEFINE_JOIN(ratio, STRSIM_INDEL)
POLARS_PLUGIN_DEFINE_JOIN(token_sort_ratio, STRSIM_TOKEN_SORT_RATIO)
POLARS_PLUGIN_DEFINE_MATCH_JOIN(levenshtein, STRSIM_LEVENSHTEIN)
POLARS_PLUGIN_DEFINE_MATCH_JOIN(jaro, STRSIM_JARO)
POLARS_PLUGIN_DEFINE_MATCH_JOIN(jaro_winkler, STRSIM_JARO_WINKLER)
POLARS_PLUGIN_DEFINE_MATCH_JOIN(jaccard, STRSIM_JACCARD)
POLARS_PLUGIN_DEFINE_MATCH_JOIN(sorensen_dice, STRSIM_SORENSEN_DICE)
POLARS_PLUGIN_DEFINE_CLUSTER(ratio, STRSIM_INDEL)
POLARS_PLUGIN_DEFINE_CLUSTER(token_sort_ratio, STRSIM_TOKEN_SORT_RATIO)
POLARS_PLUGIN_DEFINE_CLUSTER(levenshtein, STRSIM_LEVENSHTEIN)
POLARS_PLUGIN_DEFINE_CLUSTER(jaro, STRSIM_JARO)
POLARS_PLUGIN_DEFINE_CLUSTER(jaro_winkler, STRSIM_JARO_WINKLER)
POLARS_PLUGIN_DEFINE_CLUSTER(jaccard, STRSIM_JACCARD)
POLARS_PLUGIN_DEFINE_CLUSTER(sorensen_dice, STRSIM_SORENSEN_DICE)
POLARS_PLUGIN_DEFINE_QGRAM_JOIN(jaccard, STRSIM_QGRAM_JACCARD)
POLARS_PLUGIN_DEFINE_QGRAM_JOIN(sorensen_dice, STRSIM_QGRAM_SORENSEN_DICE)
POLARS_PLUGIN_DEFINE_QGRAM_JOIN(overlap, STRSIM_QGRAM_OVERLAP)
POLARS_PLUGIN_DEFINE_QGRAM_JOIN(cosine, STRSIM_QGRAM_COSINE)
POLARS_PLUGIN_DEFINE_DISTANCE_JOIN(levenshtein, STRSIM_EDIT_LEVENSHTEIN)
POLARS_PLUGIN_DEFINE_DISTANCE_JOIN(osa, STRSIM_EDIT_OSA)
POLARS_PLUGIN_DEFINE_DISTANCE_JOIN(damerau_levenshtein, STRSIM_EDIT_DAMERAU)
POLARS_PLUGIN_EXPORT(default_process, run_default_process(inputs, n_inputs, return_value),
                     field_named_after_input0(input_fields, n_fields, return_value, [](ArrowSchema *s, const char *n) { fill_named_schema(s, "u", n); }))
POLARS_PLUGIN_DEFINE_MATCH(levenshtein, STRSIM_LEVENSHTEIN)
POLARS_PLUGIN_DEFINE_MATCH(jaro, STRSIM_JARO)
POLARS_PLUGIN_DEFINE_MATCH(jaro_winkler, STRSIM_JARO_WINKLER)
POLARS_PLUGIN_DEFINE_MATCH(jaccard, STRSIM_JACCARD)
POLARS_PLUGIN_DEFINE_MATCH(sorensen_dice, STRSIM_SORENSEN_DICE)

} // extern "C"
