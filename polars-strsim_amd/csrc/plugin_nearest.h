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
    const SearchInputs in("nearest", inputs, n_inputs, true);
    const uint64_t n = in.q.rows;
    const Packed p(in.q, in.c, true);
    const uint64_t m = p.b_rows();
    StructOwned own(n, NEAREST_STRUCT);
    if (n) {
        // staging and search workspace as best match's, with 4-byte outputs, the length-ordered candidates and the fallback's
        // distance batches on top
        const uint64_t lists = std::min<uint64_t>((uint64_t)1 << 24, n * 65535u) + n;
        PipeLease lease(p.staged_bytes() + 16 * n + 84 * (n + m) + 12 * lists);
        if (strsim_nearest_host(leased_context(lease), measure, p.ao.data(), p.av.data(), n, p.bo.data(), p.bv.data(), m, 1, in.cutoff,
                                own.child<uint32_t>(0), own.child<uint32_t>(1)) != STRSIM_OK)
            fail(strsim_last_error_message());
    }
    const int64_t nulls = finish_search<uint32_t>(in.q, p.pos, n, own);
    export_struct(own, n, nulls, in.q.name.c_str(), NEAREST_STRUCT, ret);
}
