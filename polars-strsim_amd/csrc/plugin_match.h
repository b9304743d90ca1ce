// plugin_match.h -- the best_match_<measure> plugin functions: the k = 1 best candidate of every query row, as an Arrow struct
// {index: UInt32, score: Float64}.  Included by polars_plugin.cpp inside its anonymous namespace, after plugin_pack.h.
//
// Unlike the elementwise functions, the two inputs need not have the same length: input 0 is the query column (N rows, the output
// has N rows), input 1 the candidate column (any M).  Null candidates are dropped before the call and the indices map back to the
// candidate's position in input 1; a null query or a query without a candidate gives a null struct.  The strings are packed with
// the packers of the elementwise path (range_bytes / pack_range) and the search runs on a context leased from the staging pool.
#pragma once

struct StructPriv {
    ArrowArray *child[2];
    void *validity;
    const void *bufs[1];
};

struct ChildPriv {
    void *data;
    void *validity; // each child owns its copy: a consumer may move a child out of the struct (Arrow C data interface)
    const void *bufs[2];
};

void release_child_array(ArrowArray *a)
{
    if (!a || !a->release) return;
    ChildPriv *p = static_cast<ChildPriv *>(a->private_data);
    if (p) { free(p->data); free(p->validity); delete p; }
    a->release = nullptr;
}

void release_struct_array(ArrowArray *a)
{
    if (!a || !a->release) return;
    StructPriv *p = static_cast<StructPriv *>(a->private_data);
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

struct StructSchemaPriv {
    char *name;
    ArrowSchema *child[2];
    ArrowSchema *children[2];
};

void release_struct_schema(ArrowSchema *s)
{
    if (!s || !s->release) return;
    StructSchemaPriv *p = static_cast<StructSchemaPriv *>(s->private_data);
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

void fill_named_schema(ArrowSchema *s, const char *format, const char *name)
{
    fill_f64_schema(s, name);
    s->format = format;
}

// {index: UInt32, <second>: <format>}, nullable, named `name` (best match: {index: UInt32, score: Float64})
void fill_match_schema(ArrowSchema *s, const char *name, const char *second = "score", const char *format = "g")
{
    memset(s, 0, sizeof *s);
    std::unique_ptr<StructSchemaPriv> p(new StructSchemaPriv{nullptr, {nullptr, nullptr}, {nullptr, nullptr}});
    auto undo = [&p] {
        for (ArrowSchema *c : p->child) { if (c && c->release) c->release(c); free(c); }
        free(p->name);
    };
    p->name = strdup(name ? name : "");
    for (int i = 0; i < 2 && p->name; ++i) {
        p->child[i] = static_cast<ArrowSchema *>(calloc(1, sizeof(ArrowSchema)));
        if (!p->child[i]) break;
        try {
            fill_named_schema(p->child[i], i == 0 ? "I" : format, i == 0 ? "index" : second);
        } catch (...) {
            undo();
            throw;
        }
        p->children[i] = p->child[i];
    }
    if (!p->name || !p->child[0] || !p->child[1]) { undo(); throw std::bad_alloc(); }
    s->format = "+s";
    s->name = p->name;
    s->flags = ARROW_FLAG_NULLABLE;
    s->n_children = 2;
    s->children = p->children;
    s->release = release_struct_schema;
    s->private_data = p.release();
}

// every row of `c` (nulls as empty strings) -> offsets + values; with `valid_only`, only the rows whose validity is set, and
// `pos` gets each packed row's position in `c`
void pack_column(const Column &c, bool valid_only, std::vector<uint32_t> &off, std::vector<uint8_t> &val, std::vector<uint32_t> *pos)
{
    const uint64_t bytes = range_bytes(c, 0, c.rows);
    if (bytes > 0xFFFFFFFFull) fail("best_match: a column of more than 4 GiB of string data");
    std::vector<uint32_t> o(c.rows + 1, 0);
    std::vector<uint8_t> v(bytes + 16, 0);
    if (c.rows) pack_range(c, 0, c.rows, o.data(), 0, bytes, v.data());
    if (!valid_only || !c.any_null) {
        off.swap(o);
        val.swap(v);
        if (pos) { pos->resize(c.rows); for (uint64_t r = 0; r < c.rows; ++r) (*pos)[r] = (uint32_t)r; }
        return;
    }
    off.assign(1, 0);
    val.assign(bytes + 16, 0);
    uint64_t at = 0;
    for (uint64_t r = 0; r < c.rows; ++r) {
        if (!row_valid(c, r)) continue;
        const uint32_t len = o[r + 1] - o[r];
        memcpy(val.data() + at, v.data() + o[r], len);
        at += len;
        off.push_back((uint32_t)at);
        pos->push_back((uint32_t)r);
    }
}

// Every buffer and box of a struct result, allocated before any of it is handed over; until then the destructor frees them.
// buf: index (4 bytes a row), the second child (`width` bytes a row), the struct validity, the two child validities.
struct MatchOwned {
    void *buf[5] = {};
    void *box[4] = {}; // two child arrays, the struct array, the schema
    MatchOwned(uint64_t n, size_t width)
    {
        const size_t vbytes = (n + 63) / 64 * 8;
        for (int b = 0; b < 5; ++b) buf[b] = alloc64(b == 0 ? n * 4 : (b == 1 ? n * width : vbytes));
        for (int b = 0; b < 3; ++b)
            if (!(box[b] = calloc(1, sizeof(ArrowArray)))) throw std::bad_alloc();
        if (!(box[3] = calloc(1, sizeof(ArrowSchema)))) throw std::bad_alloc();
    }
    ~MatchOwned() { for (void *x : buf) free(x); for (void *x : box) free(x); }
};

// Hands the buffers of `own` to `ret` as one struct chunk {index: UInt32, <second>: <format>} of n rows named `name`.  The
// caller has filled in the struct validity (own.buf[2], `nulls` rows clear); it is copied to both children here.
void export_match_struct(MatchOwned &own, uint64_t n, int64_t nulls, const char *name, const char *second, const char *format,
                         SeriesExport *ret)
{
    const size_t vbytes = (n + 63) / 64 * 8;
    uint8_t *const valid = static_cast<uint8_t *>(own.buf[2]);
    memcpy(own.buf[3], valid, vbytes);
    memcpy(own.buf[4], valid, vbytes);

    ArrowSchema *const schema = static_cast<ArrowSchema *>(own.box[3]);
    std::unique_ptr<StructPriv> sp(new StructPriv{{nullptr, nullptr}, valid, {nulls ? valid : nullptr}});
    std::unique_ptr<ChildPriv> cp[2];
    for (int i = 0; i < 2; ++i) cp[i].reset(new ChildPriv{own.buf[i], own.buf[3 + i], {nulls ? own.buf[3 + i] : nullptr, own.buf[i]}});
    std::unique_ptr<SeriesPriv> spr(new SeriesPriv{schema, nullptr, 1});
    spr->arrays = static_cast<ArrowArray **>(calloc(1, sizeof(ArrowArray *)));
    if (!spr->arrays) throw std::bad_alloc();
    try {
        fill_match_schema(schema, name, second, format); // (the last step that may throw)
    } catch (...) {
        free(spr->arrays);
        throw;
    }
    // ---- from here on nothing allocates or throws: hand every buffer and box to the result
    for (int i = 0; i < 2; ++i) {
        ArrowArray *ch = static_cast<ArrowArray *>(own.box[i]);
        ch->length = (int64_t)n;
        ch->null_count = nulls;
        ch->n_buffers = 2;
        ch->buffers = cp[i]->bufs;
        ch->release = release_child_array;
        ch->private_data = cp[i].release();
        sp->child[i] = ch;
    }
    ArrowArray *const arr = static_cast<ArrowArray *>(own.box[2]);
    arr->length = (int64_t)n;
    arr->null_count = nulls;
    arr->n_buffers = 1;
    arr->n_children = 2;
    arr->buffers = sp->bufs;
    arr->children = sp->child;
    arr->release = release_struct_array;
    arr->private_data = sp.release();
    spr->arrays[0] = arr;
    for (void *&x : own.buf) x = nullptr;
    for (void *&x : own.box) x = nullptr;
    ret->field = schema;
    ret->arrays = spr->arrays;
    ret->len = 1;
    ret->release = release_series;
    ret->private_data = spr.release();
}


void run_best_match(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2) fail("best_match: expected 2 input series (queries, candidates), got " + std::to_string(n_inputs));
    Column q, c;
    describe(inputs[0], q);
    describe(inputs[1], c);
    if (q.rows > 0xFFFFFFFFull) fail("best_match: more than 2^32 - 1 queries");
    if (c.rows > 0xFFFFFFFEull) fail("best_match: more than 2^32 - 2 candidates");
    const uint64_t n = q.rows;
    std::vector<uint32_t> qo, co, pos;
    std::vector<uint8_t> qv, cv;
    pack_column(q, false, qo, qv, nullptr);
    pack_column(c, true, co, cv, &pos);
    const uint64_t m = pos.size();

    // every buffer and box of the result is allocated before any of it is handed over; until then `own` frees them
    const size_t vbytes = (n + 63) / 64 * 8;
    MatchOwned own(n, 8);
    uint32_t *const idx = static_cast<uint32_t *>(own.buf[0]);
    double *const score = static_cast<double *>(own.buf[1]);
    uint8_t *const valid = static_cast<uint8_t *>(own.buf[2]);
    if (n) {
        // the lease is for its context: this call's device memory is the context's staging and search workspace (strsim_capi.cpp),
        // reserved here against the staging budget at its size -- strings, offsets, outputs, packed strings and partial lists
        const uint64_t lists = std::min<uint64_t>((uint64_t)1 << 24, n * 65535u) + n;
        const uint64_t need = 2 * (qv.size() + cv.size() + 4 * (n + m + 2)) + 12 * n + 44 * (n + m) + 12 * lists;
        PipeLease lease(need);
        strsim_ctx_t *ctx = lease.set->at(0).open(plugin_devices()[0]);
        if (strsim_best_match_host(ctx, measure, qo.data(), qv.data(), n, co.data(), cv.data(), m, 1, -__builtin_inf(), idx, score) != STRSIM_OK)
            fail(strsim_last_error_message());
    }
    int64_t nulls = 0;
    memset(valid, 0, vbytes);
    for (uint64_t r = 0; r < n; ++r) {
        const bool ok = idx[r] != 0xFFFFFFFFu && row_valid(q, r);
        if (ok) { valid[r >> 3] |= (uint8_t)(1u << (r & 7)); idx[r] = pos[idx[r]]; }
        else { ++nulls; idx[r] = 0; score[r] = 0.0; }
    }
    export_match_struct(own, n, nulls, q.name.c_str(), "score", "g", ret);
}

void best_match_entry(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    InputGuard guard{inputs, n_inputs};
    try {
        run_best_match(measure, inputs, n_inputs, ret);
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

void best_match_field_entry(ArrowSchema *input_fields, size_t n_fields, ArrowSchema *ret)
{
    const char *name = (n_fields > 0 && input_fields && input_fields[0].name) ? input_fields[0].name : "";
    try {
        fill_match_schema(ret, name);
    } catch (...) { // (no exception crosses the ABI: an unreleasable, empty schema is left behind)
        memset(ret, 0, sizeof *ret);
        g_plugin_error = "out of host memory";
    }
}
