// plugin_cdist.h -- the cdist_<measure> plugin functions: the scores of every query row against every candidate, as an Arrow
// LargeList<Float64> (one list of M scores per query).  Included by polars_plugin.cpp inside its anonymous namespace, after
// plugin_extract.h.
//
// Inputs as extract's (plugin_extract.h): input 0 the queries (N rows, the output has N rows), input 1 the candidates (any M); an
// optional input 2 is score_cutoff, one Float64 value (null or absent: no cutoff), under which a score below it is 0.0.  A null
// query gives a null list; a null candidate gives a null element (the child's validity) in every list, at its own position: no
// candidate is dropped, a null one is scored as the empty string and masked.  The queries run in slices whose matrix stays within
// CDIST_SLICE_BYTES of the context's staging; every slice lands in the result's own buffer, which the array's release callback
// frees.
#pragma once

constexpr uint64_t CDIST_SLICE_BYTES = (uint64_t)32 << 20;

struct ListSchemaPriv {
    char *name;
    ArrowSchema *child;
    ArrowSchema *children[1];
};

void release_list_schema(ArrowSchema *s)
{
    if (!s || !s->release) return;
    ListSchemaPriv *p = static_cast<ListSchemaPriv *>(s->private_data);
    if (p) {
        if (p->child && p->child->release) p->child->release(p->child);
        free(p->child);
        free(p->name);
        delete p;
    }
    s->release = nullptr;
}

// the nullable LargeList<Float64> named `name` (its child: "item", nullable)
void fill_list_f64_schema(ArrowSchema *s, const char *name)
{
    memset(s, 0, sizeof *s);
    std::unique_ptr<ListSchemaPriv> p(new ListSchemaPriv{});
    p->name = strdup(name ? name : "");
    p->child = static_cast<ArrowSchema *>(calloc(1, sizeof(ArrowSchema)));
    if (!p->name || !p->child) { free(p->name); free(p->child); throw std::bad_alloc(); }
    try {
        fill_named_schema(p->child, "g", "item");
    } catch (...) {
        free(p->name); free(p->child);
        throw;
    }
    p->children[0] = p->child;
    s->format = "+L";
    s->name = p->name;
    s->flags = ARROW_FLAG_NULLABLE;
    s->n_children = 1;
    s->children = p->children;
    s->release = release_list_schema;
    s->private_data = p.release();
}

struct ListPriv {
    void *offsets, *validity;
    ArrowArray *child;
    ArrowArray *children[1];
    const void *bufs[2];
};

void release_list_array(ArrowArray *a)
{
    if (!a || !a->release) return;
    ListPriv *p = static_cast<ListPriv *>(a->private_data);
    if (p) {
        if (p->child && p->child->release) p->child->release(p->child); // (a child moved out by the consumer has release == NULL)
        free(p->child);
        free(p->offsets);
        free(p->validity);
        delete p;
    }
    a->release = nullptr;
}

// Every buffer and box of a list result, allocated before any of it is handed over; until then the destructor frees them.
struct ListOwned {
    void *values = nullptr, *cvalid = nullptr, *offsets = nullptr, *valid = nullptr;
    void *box[4] = {}; // the child array, the list array, the schema, the array pointers
    ListOwned(uint64_t n, uint64_t m, bool child_nulls, bool list_nulls)
    {
        values = alloc64(n * m * sizeof(double));
        offsets = alloc64((n + 1) * sizeof(int64_t));
        if (child_nulls) cvalid = alloc64((n * m + 63) / 64 * 8);
        if (list_nulls) valid = alloc64((n + 63) / 64 * 8);
        if (!(box[0] = calloc(1, sizeof(ArrowArray))) || !(box[1] = calloc(1, sizeof(ArrowArray))) || !(box[2] = calloc(1, sizeof(ArrowSchema))) ||
            !(box[3] = calloc(1, sizeof(ArrowArray *))))
            throw std::bad_alloc();
    }
    ~ListOwned()
    {
        free(values); free(cvalid); free(offsets); free(valid);
        for (void *x : box) free(x);
    }
};

// Hands the buffers of `own` to `ret` as one LargeList<Float64> chunk of n lists (total elements in the child) named `name`.
void export_list_f64(ListOwned &own, uint64_t n, uint64_t total, int64_t list_nulls, int64_t child_nulls, const char *name, SeriesExport *ret)
{
    ArrowSchema *const schema = static_cast<ArrowSchema *>(own.box[2]);
    ArrowArray **const arrays = static_cast<ArrowArray **>(own.box[3]);
    std::unique_ptr<ArrayPriv> cp(new ArrayPriv{own.values, own.cvalid, {own.cvalid, own.values}, false});
    std::unique_ptr<ListPriv> lp(new ListPriv{own.offsets, own.valid, nullptr, {}, {own.valid, own.offsets}});
    std::unique_ptr<SeriesPriv> sp(new SeriesPriv{schema, arrays, 1});
    fill_list_f64_schema(schema, name); // (the last step that may throw)
    // ---- from here on nothing allocates or throws: hand every buffer and box to the result
    ArrowArray *const ch = static_cast<ArrowArray *>(own.box[0]);
    ch->length = (int64_t)total;
    ch->null_count = child_nulls;
    ch->n_buffers = 2;
    ch->buffers = cp->bufs;
    ch->release = release_f64_array;
    ch->private_data = cp.release();
    lp->child = ch;
    lp->children[0] = ch;
    ArrowArray *const arr = static_cast<ArrowArray *>(own.box[1]);
    arr->length = (int64_t)n;
    arr->null_count = list_nulls;
    arr->n_buffers = 2;
    arr->n_children = 1;
    arr->buffers = lp->bufs;
    arr->children = lp->children;
    arr->release = release_list_array;
    arr->private_data = lp.release();
    arrays[0] = arr;
    own.values = own.cvalid = own.offsets = own.valid = nullptr;
    for (void *&x : own.box) x = nullptr;
    ret->field = schema;
    ret->arrays = arrays;
    ret->len = 1;
    ret->release = release_series;
    ret->private_data = sp.release();
}

void run_cdist(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2 && n_inputs != 3)
        fail("cdist: expected 2 input series (queries, candidates) and an optional score_cutoff, got " + std::to_string(n_inputs));
    const SearchInputs in("cdist", inputs, n_inputs, false);
    const double cutoff = extract_cutoff(inputs, n_inputs);
    const uint64_t n = in.q.rows, m = in.c.rows;
    if (m && n > (uint64_t)0x7FFFFFFFFFFFFFFFll / 8 / m) fail("cdist: the matrix is too large");
    const Packed p(in.q, in.c, false);
    ListOwned own(n, m, in.c.any_null, in.q.any_null);
    double *const values = static_cast<double *>(own.values);
    if (n && m) {
        const uint64_t slice = std::max<uint64_t>(1, CDIST_SLICE_BYTES / (m * sizeof(double)));
        // strings and offsets, a slice's matrix, the packed strings and the fallback's columns
        PipeLease lease(p.staged_bytes() + std::min(n, slice) * m * sizeof(double) + 44 * (n + m) + 16 * 8 * std::max(n, m));
        strsim_ctx_t *const ctx = leased_context(lease);
        for (uint64_t r0 = 0; r0 < n; r0 += slice) {
            const uint64_t rows = std::min(slice, n - r0);
            if (strsim_cdist_host(ctx, measure, p.ao.data() + r0, p.av.data(), rows, p.bo.data(), p.bv.data(), m, cutoff, values + r0 * m, m) != STRSIM_OK)
                fail(strsim_last_error_message());
        }
    }
    int64_t *const off = static_cast<int64_t *>(own.offsets);
    for (uint64_t r = 0; r <= n; ++r) off[r] = (int64_t)(r * m);
    int64_t list_nulls = 0, child_nulls = 0;
    if (own.valid) {
        uint8_t *const valid = static_cast<uint8_t *>(own.valid);
        memset(valid, 0, (n + 63) / 64 * 8);
        for (uint64_t r = 0; r < n; ++r) {
            if (row_valid(in.q, r)) valid[r >> 3] |= (uint8_t)(1u << (r & 7));
            else ++list_nulls;
        }
    }
    if (own.cvalid) {
        uint8_t *const cvalid = static_cast<uint8_t *>(own.cvalid);
        memset(cvalid, 0, (n * m + 63) / 64 * 8);
        std::vector<uint8_t> ok(m);
        int64_t per_row = 0;
        for (uint64_t j = 0; j < m; ++j) { ok[j] = row_valid(in.c, j) ? 1 : 0; per_row += !ok[j]; }
        for (uint64_t r = 0; r < n; ++r)
            for (uint64_t j = 0; j < m; ++j) {
                const uint64_t x = r * m + j;
                if (ok[j]) cvalid[x >> 3] |= (uint8_t)(1u << (x & 7));
                else values[x] = 0.0;
            }
        child_nulls = per_row * (int64_t)n;
    }
    export_list_f64(own, n, n * m, list_nulls, child_nulls, in.q.name.c_str(), ret);
}
