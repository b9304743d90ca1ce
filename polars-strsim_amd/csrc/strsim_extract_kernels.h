// strsim_extract_kernels.h -- the kernel of strsim_extract_device (the shared rules are in strsim_extract.h; DESIGN.md section
// 17).  Included by strsim_kernels.hip inside namespace strsim, after strsim_nearest_kernels.h: the strings are packed by
// k_match_pack, put in length order by k_nearest_hist / _scan / _scatter, the partial lists are reduced by k_match_merge and the
// fallback is folded by k_match_fold_cols / _rows.
//
//   k_extract_lane<K>   search_sweep_lane (strsim_nearest_kernels.h: one sweep, two rule sets) under ExtractRules
//                       (strsim_extract.h): the running top-K holds (rank, j).  The rank table (8.3 KB) is copied into LDS once
//                       per workgroup first: a pair costs one LDS read instead of an f64 division.  The partial lists carry
//                       their f64 scores (epilogue_indel of the rank's representative pair).
#pragma once

// Grid and arguments as k_nearest_lane; rlimit >= 1 is the number of admissible ranks (extract_rank_limit).
template <int K>
__global__ __launch_bounds__(MATCH_BLOCK) void k_extract_lane(const uint32_t *__restrict__ qwords, const uint32_t *__restrict__ qmeta,
                                                              const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qstart,
                                                              uint32_t nq, const uint32_t *__restrict__ sw, const uint32_t *__restrict__ sm,
                                                              const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ cstart,
                                                              const ExtractTable *__restrict__ tab, uint32_t rlimit,
                                                              double *__restrict__ pscore, uint32_t *__restrict__ pidx)
{
    __shared__ uint32_t s_words[EXTRACT_TAB_WORDS];
    {
        const uint32_t *const src = reinterpret_cast<const uint32_t *>(tab->rank);
        for (uint32_t x = threadIdx.x; x < EXTRACT_TAB_WORDS; x += MATCH_BLOCK) s_words[x] = src[x];
    }
    __syncthreads();
    const uint16_t *const s_rank = reinterpret_cast<const uint16_t *>(s_words);

    search_sweep_lane<ExtractRules, K>(ExtractRules{s_rank, tab->rep, rlimit}, qwords, qmeta, qperm, qstart, nq, sw, sm, sidx, cstart, pscore,
                                       pidx);
}
