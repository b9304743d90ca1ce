// plugin_common.h -- the hamming / prefix / postfix / lcs_seq plugin functions, three a kind (strsim_common_host,
// strsim_common_distance_host and strsim_common_count_host of strsim_amd.h).  Included by polars_plugin.cpp inside its anonymous
// namespace, after plugin_distance.h, whose two bodies they run through:
//   <kind>             the normalised similarity, one Float64 ("g") chunk (run_similarity_by)
//   <kind>_distance    the distance, one UInt32 ("I") chunk, with the optional max_distance input 2 (run_distance_by)
//   <kind>_similarity  the count, one UInt32 chunk; it takes no cutoff, and a third input is an error
// Shape rule, literal broadcast, null handling and error messages are those of the functions of plugin_distance.h.
#pragma once

void run_common(int kind, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    run_similarity_by(
        [kind](strsim_ctx_t *c, const uint32_t *ao, const uint8_t *av, uint64_t ar, const uint32_t *bo, const uint8_t *bv, uint64_t br,
               double *out, uint64_t n) { return strsim_common_host(c, kind, ao, av, ar, bo, bv, br, out, n); },
        inputs, n_inputs, ret);
}

void run_common_distance(int kind, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    run_distance_by(
        [kind](strsim_ctx_t *c, const uint32_t *ao, const uint8_t *av, uint64_t ar, const uint32_t *bo, const uint8_t *bv, uint64_t br,
               uint32_t k, uint32_t *out, uint64_t n) { return strsim_common_distance_host(c, kind, ao, av, ar, bo, bv, br, k, out, n); },
        inputs, n_inputs, ret);
}

void run_common_count(int kind, SeriesExport *inputs, size_t n_inputs, SeriesExport *ret)
{
    if (n_inputs != 2) fail("expected 2 input series, got " + std::to_string(n_inputs));
    run_distance_by(
        [kind](strsim_ctx_t *c, const uint32_t *ao, const uint8_t *av, uint64_t ar, const uint32_t *bo, const uint8_t *bv, uint64_t br,
               uint32_t, uint32_t *out, uint64_t n) { return strsim_common_count_host(c, kind, ao, av, ar, bo, bv, br, out, n); },
        inputs, n_inputs, ret);
}
