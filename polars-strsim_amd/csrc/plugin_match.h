// plugin_match.h -- the best_match_<measure> plugin functions: the k = 1 best candidate of every query row, as an Arrow struct
// {index: UInt32, score: Float64}.  Included by polars_plugin.cpp inside its anonymous namespace, after plugin_pack.h.
//
// This file also holds what the other non-pipelined families (plugin_distance.h, plugin_partial.h, plugin_nearest.h) share with it:
// the struct result, the packing of whole columns and the lease of a context.
//
// Unlike the elementwise functions, the two inputs need not have the same length: input 0 is the query column (N rows, the output
// has N rows), input 1 the candidate column (any M).  Null candidates are dropped before the call and the indices map back to the
// candidate's position in input 1; a null query or a query without a candidate gives a null struct.  The strings are packed with
// the packers of the elementwise path (range_bytes / pack_range) and the search runs on a context leased from the staging pool.
#pragma once

// ---- a struct result of up to STRUCT_MAX_CHILDREN primitive children (best match, nearest, partial_ratio_alignment) ----
constexpr int STRUCT_MAX_CHILDREN = 5;
struct StructShape {
    int n;
    const char *name[STRUCT_MAX_CHILDREN];
    const char *format[STRUCT_MAX_CHILDREN]; // "g" (Float64, 8 bytes a row) or "I" (UInt32, 4)
};
const StructShape MATCH_STRUCT = {2, {"index", "score"}, {"I", "g"}};
const StructShape NEAREST_STRUCT = {2, {"index", "distance"}, {"I", "I"}};
const StructShape PARTIAL_STRUCT = {5, {"score", "src_start", "src_end", "dest_start", "dest_end"}, {"g", "I", "I", "I", "I"}};

struct StructPriv {
    int n;
    ArrowArray *child[STRUCT_MAX_CHILDREN];
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
        for (int i = 0; i < p->n; ++i) {
            ArrowArray *c = p->child[i];
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
    ArrowSchema *child[STRUCT_MAX_CHILDREN];    // what this schema owns
    ArrowSchema *children[STRUCT_MAX_CHILDREN]; // what ArrowSchema::children points at
    void drop()
    {
        for (ArrowSchema *c : child) { if (c && c->release) c->release(c); free(c); }
        free(name);
    }
};

void release_struct_schema(ArrowSchema *s)
{
    if (!s || !s->release) return;
    StructSchemaPriv *p = static_cast<StructSchemaPriv *>(s->private_data);
    if (p) { p->drop(); delete p; }
    s->release = nullptr;
}

// the nullable struct `shape`, named `name`
void fill_struct_schema(ArrowSchema *s, const char *name, const StructShape &shape)
{
    memset(s, 0, sizeof *s);
    std::unique_ptr<StructSchemaPriv> p(new StructSchemaPriv{});
    p->name = strdup(name ? name : "");
    bool ok = p->name != nullptr;
    for (int i = 0; i < shape.n && ok; ++i) {
        p->child[i] = static_cast<ArrowSchema *>(calloc(1, sizeof(ArrowSchema)));
        if (!p->child[i]) { ok = false; break; }
        try {
            fill_named_schema(p->child[i], shape.format[i], shape.name[i]);
        } catch (...) {
            p->drop();
            throw;
        }
        p->children[i] = p->child[i];
    }
    if (!ok) { p->drop(); throw std::bad_alloc(); }
    s->format = "+s";
    s->name = p->name;
    s->flags = ARROW_FLAG_NULLABLE;
    s->n_children = shape.n;
    s->children = p->children;
    s->release = release_struct_schema;
    s->private_data = p.release();
}

// Every buffer and box of a struct result of n rows, allocated before any of it is handed over; until then the destructor frees
// them.
struct StructOwned {
    void *data[STRUCT_MAX_CHILDREN] = {};
    void *cvalid[STRUCT_MAX_CHILDREN] = {}; // the children's copies of the validity (export_struct fills them)
    void *valid = nullptr;                  // the struct's validity: the caller fills it
    void *box[STRUCT_MAX_CHILDREN + 2] = {}; // the child arrays, then the struct array and the schema
    StructOwned(uint64_t n, const StructShape &shape)
    {
        const size_t vbytes = (n + 63) / 64 * 8;
        for (int i = 0; i < shape.n; ++i) {
            data[i] = alloc64(n * (shape.format[i][0] == 'g' ? 8 : 4));
            cvalid[i] = alloc64(vbytes);
        }
        valid = alloc64(vbytes);
        for (int b = 0; b <= shape.n; ++b)
            if (!(box[b] = calloc(1, sizeof(ArrowArray)))) throw std::bad_alloc();
        if (!(box[shape.n + 1] = calloc(1, sizeof(ArrowSchema)))) throw std::bad_alloc();
    }
    ~StructOwned()
    {
        for (void *x : data) free(x);
        for (void *x : cvalid) free(x);
        free(valid);
        for (void *x : box) free(x);
    }
    template <class T> T *child(int i) const { return static_cast<T *>(data[i]); }
};

// Hands the buffers of `own` to `ret` as one struct chunk `shape` of n rows named `name`.  The caller has filled in the children
// and the struct validity (own.valid, `nulls` rows clear); every child gets its copy of it here.
void export_struct(StructOwned &own, uint64_t n, int64_t nulls, const char *name, const StructShape &shape, SeriesExport *ret)
{
    const size_t vbytes = (n + 63) / 64 * 8;
    for (int i = 0; i < shape.n; ++i) memcpy(own.cvalid[i], own.valid, vbytes);

    ArrowSchema *const schema = static_cast<ArrowSchema *>(own.box[shape.n + 1]);
    std::unique_ptr<StructPriv> sp(new StructPriv{shape.n, {}, own.valid, {nulls ? own.valid : nullptr}});
    std::unique_ptr<ChildPriv> cp[STRUCT_MAX_CHILDREN];
    for (int i = 0; i < shape.n; ++i)
        cp[i].reset(new ChildPriv{own.data[i], own.cvalid[i], {nulls ? own.cvalid[i] : nullptr, own.data[i]}});
    std::unique_ptr<SeriesPriv> spr(new SeriesPriv{schema, nullptr, 1});
    spr->arrays = static_cast<ArrowArray **>(calloc(1, sizeof(ArrowArray *)));
    if (!spr->arrays) throw std::bad_alloc();
    try {
        fill_struct_schema(schema, name, shape); // (the last step that may throw)
    } catch (...) {
        free(spr->arrays);
        throw;
    }
    // ---- from here on nothing allocates or throws: hand every buffer and box to the result
    for (int i = 0; i < shape.n; ++i) {
        ArrowArray *ch = static_cast<ArrowArray *>(own.box[i]);
        ch->length = (int64_t)n;
        ch->null_count = nulls;
        ch->n_buffers = 2;
        ch->buffers = cp[i]->bufs;
        ch->release = release_child_array;
        ch->private_data = cp[i].release();
        sp->child[i] = ch;
    }
    ArrowArray *const arr = static_cast<ArrowArray *>(own.box[shape.n]);
    arr->length = (int64_t)n;
    arr->null_count = nulls;
    arr->n_buffers = 1;
    arr->n_children = shape.n;
    arr->buffers = sp->bufs;
    arr->children = sp->child;
    arr->release = release_struct_array;
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

// ---- the host side of a call that is not pipelined: both columns packed whole, a context leased for the call ----
struct Packed {
    std::vector<uint32_t> ao, bo, pos; // pos: with drop_null_b, each packed row of b's position in the column
    std::vector<uint8_t> av, bv;
    Packed(const Column &a, const Column &b, bool drop_null_b)
    {
        pack_column(a, false, ao, av, nullptr);
        pack_column(b, drop_null_b, bo, bv, drop_null_b ? &pos : nullptr);
    }
    uint64_t a_rows() const { return ao.size() - 1; }
    uint64_t b_rows() const { return bo.size() - 1; }
    // device memory of the staged strings and offsets (the context's staging, strsim_capi.cpp), for the lease
    uint64_t staged_bytes() const { return 2 * (av.size() + bv.size() + 4 * (ao.size() + bo.size())); }
};

// The lease is for its context: a call's device memory is the context's staging and workspaces (strsim_capi.cpp), reserved against
// the staging budget at the size the caller estimated.
strsim_ctx_t *leased_context(PipeLease &lease) { return lease.set->at(0).open(plugin_devices()[0]); }

// ---- the two search families (best match, nearest): input 0 the queries, input 1 the candidates ----
// The value of a length-1, non-null UInt32 series (Polars pickles keyword arguments; a literal series needs no parsing); `what`
// names the argument in the messages.
uint32_t uint32_literal(const SeriesExport &s, const std::string &what)
{
    if (!s.field || !s.field->format || strcmp(s.field->format, "I") != 0)
        fail(what + " must be a UInt32 series, got Arrow format '" + (s.field && s.field->format ? s.field->format : "") + "'");
    uint64_t rows = 0;
    const ArrowArray *one = nullptr;
    for (size_t i = 0; i < s.len; ++i) {
        const ArrowArray *a = s.arrays[i];
        if (!a || a->length == 0) continue;
        rows += (uint64_t)a->length;
        one = a;
    }
    if (rows != 1) fail(what + " must be a single value, got " + std::to_string(rows) + " rows");
    const uint8_t *valid = one->n_buffers > 0 ? static_cast<const uint8_t *>(one->buffers[0]) : nullptr;
    if (one->null_count > 0 || (valid && !bit_at(valid, one->offset))) fail(what + " must not be null");
    if (one->n_buffers < 2 || !one->buffers[1]) fail(what + ": the UInt32 series has no data buffer");
    return static_cast<const uint32_t *>(one->buffers[1])[one->offset];
}

// max_distance from input 2 of the distance and nearest functions (STRSIM_DISTANCE_UNBOUNDED without one)
uint32_t distance_cutoff(SeriesExport *inputs, size_t n_inputs)
{
    if (n_inputs == 2) return STRSIM_DISTANCE_UNBOUNDED;
    return uint32_literal(inputs[2], "max_distance");
}

struct SearchInputs {
    Column q, c;
    uint32_t cutoff = 0; // max_distance of input 2 (nearest)
    SearchInputs(const char *who, SeriesExport *inputs, size_t n_inputs, bool with_cutoff)
    {
        describe(inputs[0], q);
        describe(inputs[1], c);
        if (with_cutoff) cutoff = distance_cutoff(inputs, n_inputs);
        if (q.rows > 0xFFFFFFFFull) fail(std::string(who) + ": more than 2^32 - 1 queries");
        if (c.rows > 0xFFFFFFFEull) fail(std::string(who) + ": more than 2^32 - 2 candidates");
    }
};

// The struct validity of a search result and the indices mapped back to rows of input 1: a null query or a query without a
// candidate gives a null struct (children zeroed).  -> the null count
template <class T> int64_t finish_search(const Column &q, const std::vector<uint32_t> &pos, uint64_t n, StructOwned &own)
{
    uint32_t *const idx = own.child<uint32_t>(0);
    T *const second = own.child<T>(1);
    uint8_t *const valid = static_cast<uint8_t *>(own.valid);
    int64_t nulls = 0;
    memset(valid, 0, (n + 63) / 64 * 8);
    for (uint64_t r = 0; r < n; ++r) {
        const bool ok = idx[r] != 0xFFFFFFFFu && row_valid(q, r);
        if (ok) { valid[r >> 3] |= (uint8_t)(1u << (r & 7)); idx[r] = pos[idx[r]]; }
        else { ++nulls; idx[r] = 0; second[r] = 0; }
    }
    return nulls;
}

void run_best_match(int measure, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2) fail("best_match: expected 2 input series (queries, candidates), got " + std::to_string(n_inputs));
    const SearchInputs in("best_match", inputs, n_inputs, false);
    const uint64_t n = in.q.rows;
    const Packed p(in.q, in.c, true);
    const uint64_t m = p.b_rows();
    StructOwned own(n, MATCH_STRUCT);
    if (n) {
        // strings, offsets, outputs, packed strings and partial lists
        const uint64_t lists = std::min<uint64_t>((uint64_t)1 << 24, n * 65535u) + n;
        PipeLease lease(p.staged_bytes() + 12 * n + 44 * (n + m) + 12 * lists);
        if (strsim_best_match_host(leased_context(lease), measure, p.ao.data(), p.av.data(), n, p.bo.data(), p.bv.data(), m, 1, -__builtin_inf(),
                                   own.child<uint32_t>(0), own.child<double>(1)) != STRSIM_OK)
            fail(strsim_last_error_message());
    }
    const int64_t nulls = finish_search<double>(in.q, p.pos, n, own);
    export_struct(own, n, nulls, in.q.name.c_str(), MATCH_STRUCT, ret);
}
