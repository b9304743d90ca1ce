// plugin_join.h -- the join_ratio / join_token_sort_ratio plugin functions: every candidate of a query row that scores at least
// score_cutoff, as an Arrow LargeList<Struct{index: UInt32, score: Float64}> (one list of hits per query, in ascending candidate
// index).  Included by polars_plugin.cpp inside its anonymous namespace, after plugin_cdist.h: the struct export of plugin_match.h
// under the list export of plugin_cdist.h.
//
// Inputs as extract's (plugin_extract.h): input 0 the queries (N rows, the output has N rows), input 1 the candidates (any M; null
// candidates are dropped before the call and the indices map back to rows of input 1, so they are never matched); an optional
// input 2 is score_cutoff, parsed by extract_cutoff (null or absent: every pair).  A null query gives a null list; a query without
// a hit gives an empty one.  The call is strsim_join_host: once to count (capacity 0), once more with exactly nnz slots.
//
// The match_join_<measure> functions (the five reference measures; input 2 is min_score) are the same flow over
// strsim_match_join_host: run_join takes the host entry point to call.  The qgram_join_<kind> functions (plugin_qgram_join.h) are
// the same flow again over strsim_qgram_join_host: run_join_call takes the call itself, with whatever the family binds to it.  The
// distance_join_<kind> functions (plugin_distance_join.h) carry a UInt32 distance where the score stands: run_join_values takes the
// type of the value, the struct's shape and the cutoff as the family parsed it.
#pragma once

// the nullable LargeList<Struct `shape`> named `name` (its child: "item")
void fill_list_struct_schema_of(ArrowSchema *s, const char *name, const StructShape &shape)
{
    memset(s, 0, sizeof *s);
    std::unique_ptr<ListSchemaPriv> p(new ListSchemaPriv{});
    p->name = strdup(name ? name : "");
    p->child = static_cast<ArrowSchema *>(calloc(1, sizeof(ArrowSchema)));
    if (!p->name || !p->child) { free(p->name); free(p->child); throw std::bad_alloc(); }
    try {
        fill_struct_schema(p->child, "item", shape);
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

// the nullable LargeList<Struct{index, score}> named `name`
void fill_list_struct_schema(ArrowSchema *s, const char *name) { fill_list_struct_schema_of(s, name, MATCH_STRUCT); }

// Every buffer and box of a join result, allocated before any of it is handed over; until then the destructor frees them.
struct JoinOwned {
    void *index = nullptr, *score = nullptr, *offsets = nullptr, *valid = nullptr;
    void *box[6] = {}; // the two primitive arrays, the struct array, the list array, the schema, the array pointers
    JoinOwned(uint64_t n, bool list_nulls)
    {
        offsets = alloc64((n + 1) * sizeof(int64_t));
        if (list_nulls) valid = alloc64((n + 63) / 64 * 8);
        for (int b = 0; b < 4; ++b)
            if (!(box[b] = calloc(1, sizeof(ArrowArray)))) throw std::bad_alloc();
        if (!(box[4] = calloc(1, sizeof(ArrowSchema))) || !(box[5] = calloc(1, sizeof(ArrowArray *)))) throw std::bad_alloc();
    }
    void room(uint64_t nnz, size_t value_bytes = sizeof(double)) // (score: the hits' values, f64 scores or uint32 distances)
    {
        index = alloc64(nnz * sizeof(uint32_t));
        score = alloc64(nnz * value_bytes);
    }
    ~JoinOwned()
    {
        free(index); free(score); free(offsets); free(valid);
        for (void *x : box) free(x);
    }
};

// Hands the buffers of `own` to `ret` as one LargeList<Struct `shape`> chunk of n lists (nnz structs in the child) named `name`.
void export_list_struct(JoinOwned &own, uint64_t n, uint64_t nnz, int64_t list_nulls, const char *name, SeriesExport *ret,
                        const StructShape &shape = MATCH_STRUCT)
{
    ArrowSchema *const schema = static_cast<ArrowSchema *>(own.box[4]);
    ArrowArray **const arrays = static_cast<ArrowArray **>(own.box[5]);
    std::unique_ptr<ChildPriv> ci(new ChildPriv{own.index, nullptr, {nullptr, own.index}});
    std::unique_ptr<ChildPriv> cs(new ChildPriv{own.score, nullptr, {nullptr, own.score}});
    std::unique_ptr<StructPriv> st(new StructPriv{2, {}, nullptr, {nullptr}});
    std::unique_ptr<ListPriv> lp(new ListPriv{own.offsets, own.valid, nullptr, {}, {own.valid, own.offsets}});
    std::unique_ptr<SeriesPriv> sp(new SeriesPriv{schema, arrays, 1});
    fill_list_struct_schema_of(schema, name, shape); // (the last step that may throw)
    // ---- from here on nothing allocates or throws: hand every buffer and box to the result
    ChildPriv *const cp[2] = {ci.release(), cs.release()};
    for (int i = 0; i < 2; ++i) {
        ArrowArray *const ch = static_cast<ArrowArray *>(own.box[i]);
        ch->length = (int64_t)nnz;
        ch->n_buffers = 2;
        ch->buffers = cp[i]->bufs;
        ch->release = release_child_array;
        ch->private_data = cp[i];
        st->child[i] = ch;
    }
    ArrowArray *const sa = static_cast<ArrowArray *>(own.box[2]);
    sa->length = (int64_t)nnz;
    sa->n_buffers = 1;
    sa->n_children = 2;
    sa->buffers = st->bufs;
    sa->children = st->child;
    sa->release = release_struct_array;
    sa->private_data = st.release();
    lp->child = sa;
    lp->children[0] = sa;
    ArrowArray *const arr = static_cast<ArrowArray *>(own.box[3]);
    arr->length = (int64_t)n;
    arr->null_count = list_nulls;
    arr->n_buffers = 2;
    arr->n_children = 1;
    arr->buffers = lp->bufs;
    arr->children = lp->children;
    arr->release = release_list_array;
    arr->private_data = lp.release();
    arrays[0] = arr;
    own.index = own.score = own.offsets = own.valid = nullptr;
    for (void *&x : own.box) x = nullptr;
    ret->field = schema;
    ret->arrays = arrays;
    ret->len = 1;
    ret->release = release_series;
    ret->private_data = sp.release();
}

// strsim_join_host or strsim_match_join_host
typedef int (*JoinHostFn)(strsim_ctx_t *, int, const uint32_t *, const uint8_t *, uint64_t, const uint32_t *, const uint8_t *, uint64_t, double, uint32_t,
                          uint64_t, uint64_t *, uint32_t *, double *, uint64_t *);

// join_host(ctx, q_off, q_val, q_rows, c_off, c_val, c_rows, cutoff, capacity, indptr, index, value, &nnz): the family's host entry
// point with its scorer bound and no flags.  T: the type of a hit's value (the second child of `shape`); parse_cutoff() gives the
// family's cutoff (behind the columns' own checks, as the messages are ordered).
template <class T, class ParseCutoff, class JoinHost>
void run_join_values(JoinHost join_host, ParseCutoff parse_cutoff, const StructShape &shape, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    const SearchInputs in("join", inputs, n_inputs, false);
    const auto cutoff = parse_cutoff();
    const uint64_t n = in.q.rows;
    const Packed p(in.q, in.c, true);
    const uint64_t m = p.b_rows();
    JoinOwned own(n, in.q.any_null);
    std::vector<uint64_t> indptr(n + 1, 0);
    uint64_t nnz = 0;
    if (n) {
        // staging and workspace of the count call, then of the fill: strings and offsets, indptr, packed strings, length order and
        // counts, the fallback's columns; the outputs once nnz is known
        PipeLease lease(2 * p.staged_bytes() + 16 * n + 84 * (n + m) + 4 * 65 * n + 16 * 8 * std::max(n, m));
        strsim_ctx_t *const ctx = leased_context(lease);
        if (join_host(ctx, p.ao.data(), p.av.data(), n, p.bo.data(), p.bv.data(), m, cutoff, (uint64_t)0, indptr.data(), (uint32_t *)nullptr,
                      (T *)nullptr, &nnz) != STRSIM_OK)
            fail(strsim_last_error_message());
        own.room(nnz, sizeof(T));
        if (nnz && join_host(ctx, p.ao.data(), p.av.data(), n, p.bo.data(), p.bv.data(), m, cutoff, nnz, indptr.data(),
                             static_cast<uint32_t *>(own.index), static_cast<T *>(own.score), &nnz) != STRSIM_OK)
            fail(strsim_last_error_message());
    } else {
        own.room(0, sizeof(T));
    }
    // the hits of a null query (scored as the empty string) are dropped: the lists are compacted in place
    uint32_t *const index = static_cast<uint32_t *>(own.index);
    T *const score = static_cast<T *>(own.score);
    int64_t *const off = static_cast<int64_t *>(own.offsets);
    uint8_t *const valid = static_cast<uint8_t *>(own.valid);
    if (valid) memset(valid, 0, (n + 63) / 64 * 8);
    int64_t list_nulls = 0;
    uint64_t at = 0;
    off[0] = 0;
    for (uint64_t r = 0; r < n; ++r) {
        if (row_valid(in.q, r)) {
            if (valid) valid[r >> 3] |= (uint8_t)(1u << (r & 7));
            for (uint64_t x = indptr[r]; x < indptr[r + 1]; ++x, ++at) {
                index[at] = p.pos[index[x]];
                score[at] = score[x];
            }
        } else {
            ++list_nulls;
        }
        off[r + 1] = (int64_t)at;
    }
    export_list_struct(own, n, at, list_nulls, in.q.name.c_str(), ret, shape);
}

// The families whose hits carry an f64 score: an optional input 2 is the cutoff (extract_cutoff).
template <class JoinHost>
void run_join_call(JoinHost join_host, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2 && n_inputs != 3)
        fail("join: expected 2 input series (queries, candidates) and an optional score_cutoff, got " + std::to_string(n_inputs));
    run_join_values<double>(join_host, [&] { return extract_cutoff(inputs, n_inputs); }, MATCH_STRUCT, inputs, n_inputs, ret);
}

void run_join(JoinHostFn join_host, int scorer, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    run_join_call(
        [=](strsim_ctx_t *ctx, const uint32_t *qo, const uint8_t *qv, uint64_t n, const uint32_t *co, const uint8_t *cv, uint64_t m, double cutoff,
            uint64_t capacity, uint64_t *indptr, uint32_t *index, double *score, uint64_t *nnz) {
            return join_host(ctx, scorer, qo, qv, n, co, cv, m, cutoff, 0u, capacity, indptr, index, score, nnz);
        },
        inputs, n_inputs, ret);
}
