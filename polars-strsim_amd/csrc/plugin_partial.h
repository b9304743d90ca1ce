// plugin_partial.h -- the partial_ratio_alignment plugin function: the partial ratio of every row with the window that won, as one
// Arrow struct chunk {score: Float64, src_start, src_end, dest_start, dest_end: UInt32} named after input 0 (src = input 0, dest =
// input 1; half-open spans in Unicode scalar values).  Included by polars_plugin.cpp inside its anonymous namespace, after
// plugin_distance.h.
//
// Shape rule, literal broadcast, null handling (null in, null out) and error messages of the similarity functions.  The strings
// are packed with the best-match packers and run through strsim_partial_alignment_host on a context leased from the staging pool;
// the struct is built the way best match builds its own (every child owns its copy of the validity).  Bypasses the small-call
// combiner.
#pragma once

constexpr int PARTIAL_CHILDREN = 5;
const char *const PARTIAL_CHILD_NAME[PARTIAL_CHILDREN] = {"score", "src_start", "src_end", "dest_start", "dest_end"};

struct PartialStructPriv {
    ArrowArray *child[PARTIAL_CHILDREN];
    void *validity;
    const void *bufs[1];
};

void release_partial_struct_array(ArrowArray *a)
{
    if (!a || !a->release) return;
    PartialStructPriv *p = static_cast<PartialStructPriv *>(a->private_data);
    if (p) {
        for (ArrowArray *c : p->child) {
            if (c && c->release) c->release(c); // (a child moved out by the consumer has release == NULL)
            free(c);
        }
        free(p->validity);
        delete p;
    }
    a->release = nullptr;
}

struct PartialSchemaPriv {
    char *name;
    ArrowSchema *child[PARTIAL_CHILDREN];
    ArrowSchema *children[PARTIAL_CHILDREN];
};

void release_partial_schema(ArrowSchema *s)
{
    if (!s || !s->release) return;
    PartialSchemaPriv *p = static_cast<PartialSchemaPriv *>(s->private_data);
    if (p) {
        for (ArrowSchema *c : p->child) {
            if (c && c->release) c->release(c);
            free(c);
        }
        free(p->name);
        delete p;
    }
    s->release = nullptr;
}

void fill_partial_schema(ArrowSchema *s, const char *name)
{
    memset(s, 0, sizeof *s);
    std::unique_ptr<PartialSchemaPriv> p(new PartialSchemaPriv{});
    auto undo = [&p] {
        for (ArrowSchema *c : p->child) { if (c && c->release) c->release(c); free(c); }
        free(p->name);
    };
    p->name = strdup(name ? name : "");
    bool ok = p->name != nullptr;
    for (int i = 0; i < PARTIAL_CHILDREN && ok; ++i) {
        p->child[i] = static_cast<ArrowSchema *>(calloc(1, sizeof(ArrowSchema)));
        if (!p->child[i]) { ok = false; break; }
        try {
            fill_named_schema(p->child[i], i == 0 ? "g" : "I", PARTIAL_CHILD_NAME[i]);
        } catch (...) {
            undo();
            throw;
        }
        p->children[i] = p->child[i];
    }
    if (!ok) { undo(); throw std::bad_alloc(); }
    s->format = "+s";
    s->name = p->name;
    s->flags = ARROW_FLAG_NULLABLE;
    s->n_children = PARTIAL_CHILDREN;
    s->children = p->children;
    s->release = release_partial_schema;
    s->private_data = p.release();
}

// Every buffer and box of the result, allocated before any of it is handed over; until then the destructor frees them.
struct PartialOwned {
    void *data[PARTIAL_CHILDREN] = {};
    void *cvalid[PARTIAL_CHILDREN] = {};
    void *valid = nullptr;
    void *box[PARTIAL_CHILDREN + 2] = {}; // the child arrays, the struct array, the schema
    explicit PartialOwned(uint64_t n)
    {
        const size_t vbytes = (n + 63) / 64 * 8;
        for (int i = 0; i < PARTIAL_CHILDREN; ++i) {
            data[i] = alloc64(n * (i == 0 ? 8 : 4));
            cvalid[i] = alloc64(vbytes);
        }
        valid = alloc64(vbytes);
        for (int b = 0; b <= PARTIAL_CHILDREN; ++b)
            if (!(box[b] = calloc(1, sizeof(ArrowArray)))) throw std::bad_alloc();
        if (!(box[PARTIAL_CHILDREN + 1] = calloc(1, sizeof(ArrowSchema)))) throw std::bad_alloc();
    }
    ~PartialOwned()
    {
        for (void *x : data) free(x);
        for (void *x : cvalid) free(x);
        free(valid);
        for (void *x : box) free(x);
    }
};

void run_partial_alignment(SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2) fail("expected 2 input series, got " + std::to_string(n_inputs));
    Column col[2];
    describe(inputs[0], col[0]);
    describe(inputs[1], col[1]);
    const Column &a = col[0], &b = col[1];
    if (a.rows != b.rows && a.rows != 1 && b.rows != 1) // strsim.rs:48-52
        fail("Inputs must have the same length, or one of them must be a Utf8 literal.");
    const bool lit[2] = {a.rows == 1 && b.rows != 1, b.rows == 1};
    const uint64_t n = lit[0] ? b.rows : a.rows;
    const bool all_null = (lit[0] && !row_valid(a, 0)) || (lit[1] && !row_valid(b, 0));
    const size_t vbytes = (n + 63) / 64 * 8;

    PartialOwned own(n);
    double *const score = static_cast<double *>(own.data[0]);
    std::vector<uint32_t> span(n * 4 + 4, 0u);
    if (n != 0 && !all_null) {
        std::vector<uint32_t> ao, bo;
        std::vector<uint8_t> av, bv;
        pack_column(a, false, ao, av, nullptr);
        pack_column(b, false, bo, bv, nullptr);
        // the lease is for its context: staged strings, offsets and outputs, the work list and the wave tier's scratch
        const uint64_t need = 2 * (av.size() + bv.size() + 4 * (a.rows + b.rows + 2)) + 28 * n;
        PipeLease lease(need);
        strsim_ctx_t *ctx = lease.set->at(0).open(plugin_devices()[0]);
        if (strsim_partial_alignment_host(ctx, ao.data(), av.data(), a.rows, bo.data(), bv.data(), b.rows, score, span.data(), n) != STRSIM_OK)
            fail(strsim_last_error_message());
    } else {
        for (uint64_t r = 0; r < n; ++r) score[r] = 0.0;
    }
    uint64_t *const vw = static_cast<uint64_t *>(own.valid);
    int64_t nulls = 0;
    if ((all_null || a.any_null || b.any_null) && n != 0) nulls = build_validity(col, lit, n, all_null, 1, vw, nullptr);
    else memset(own.valid, 0xFF, vbytes);
    for (uint64_t r = 0; r < n; ++r) { // (values under nulls: 0, never observable)
        const bool ok = (vw[r >> 6] >> (r & 63)) & 1u;
        if (!ok) score[r] = 0.0;
        for (int k = 0; k < 4; ++k) static_cast<uint32_t *>(own.data[1 + k])[r] = ok ? span[4 * r + k] : 0u;
    }
    for (int i = 0; i < PARTIAL_CHILDREN; ++i) memcpy(own.cvalid[i], own.valid, vbytes);

    ArrowSchema *const schema = static_cast<ArrowSchema *>(own.box[PARTIAL_CHILDREN + 1]);
    std::unique_ptr<PartialStructPriv> sp(new PartialStructPriv{{}, own.valid, {nulls ? own.valid : nullptr}});
    std::unique_ptr<ChildPriv> cp[PARTIAL_CHILDREN];
    for (int i = 0; i < PARTIAL_CHILDREN; ++i)
        cp[i].reset(new ChildPriv{own.data[i], own.cvalid[i], {nulls ? own.cvalid[i] : nullptr, own.data[i]}});
    std::unique_ptr<SeriesPriv> spr(new SeriesPriv{schema, nullptr, 1});
    spr->arrays = static_cast<ArrowArray **>(calloc(1, sizeof(ArrowArray *)));
    if (!spr->arrays) throw std::bad_alloc();
    try {
        fill_partial_schema(schema, a.name.c_str()); // (the last step that may throw)
    } catch (...) {
        free(spr->arrays);
        throw;
    }
    // ---- from here on nothing allocates or throws: hand every buffer and box to the result
    for (int i = 0; i < PARTIAL_CHILDREN; ++i) {
        ArrowArray *ch = static_cast<ArrowArray *>(own.box[i]);
        ch->length = (int64_t)n;
        ch->null_count = nulls;
        ch->n_buffers = 2;
        ch->buffers = cp[i]->bufs;
        ch->release = release_child_array;
        ch->private_data = cp[i].release();
        sp->child[i] = ch;
    }
    ArrowArray *const arr = static_cast<ArrowArray *>(own.box[PARTIAL_CHILDREN]);
    arr->length = (int64_t)n;
    arr->null_count = nulls;
    arr->n_buffers = 1;
    arr->n_children = PARTIAL_CHILDREN;
    arr->buffers = sp->bufs;
    arr->children = sp->child;
    arr->release = release_partial_struct_array;
    arr->private_data = sp.release();
    spr->arrays[0] = arr;
    for (void *&x : own.data) x = nullptr;
    for (void *&x : own.cvalid) x = nullptr;
    own.valid = nullptr;
    for (void *&x : own.box) x = nullptr;
    ret->field = schema;
    ret->arrays = spr->arrays;
    ret->len = 1;
    ret->release = release_series;
    ret->private_data = spr.release();
}

void partial_alignment_entry(SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    InputGuard guard{inputs, n_inputs};
    try {
        run_partial_alignment(inputs, n_inputs, ret);
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

void partial_alignment_field_entry(ArrowSchema *input_fields, size_t n_fields, ArrowSchema *ret)
{
    const char *name = (n_fields > 0 && input_fields && input_fields[0].name) ? input_fields[0].name : "";
    try {
        fill_partial_schema(ret, name);
    } catch (...) { // (no exception crosses the ABI: an unreleasable, empty schema is left behind)
        memset(ret, 0, sizeof *ret);
        g_plugin_error = "out of host memory";
    }
}
