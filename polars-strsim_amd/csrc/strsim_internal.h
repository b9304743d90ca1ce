// strsim_internal.h -- helpers shared by the C-ABI translation units (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>

#include "strsim_amd.h"

namespace strsim {

void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
int hip_fail(hipError_t e, const char *what);

// 64 KB of device scratch owned by the context (strsim_capi.cpp), for strsim_offsets_from_lengths' block sums
constexpr size_t SCAN_WS_WORDS = 16384;

// token_ratio, the partial token ratios and WRatio: the even ids 18 .. 26 (strsim_wratio.h)
inline bool weighted_measure(int measure) { return measure >= STRSIM_TOKEN_RATIO && measure <= STRSIM_WRATIO && (measure & 1) == 0; }

// Which measures each entry point accepts (strsim_measure_supported answers from here; so do the argument checks).
inline bool measure_accepted(int measure, int entry_point)
{
    const bool reference_five = measure >= 0 && measure < STRSIM_NUM_MEASURES;
    switch (entry_point) {
    case STRSIM_ENTRY_PAIRWISE: return reference_five || measure == STRSIM_OSA || measure == STRSIM_INDEL || measure == STRSIM_PARTIAL_RATIO ||
                                       measure == STRSIM_TOKEN_SORT_RATIO || measure == STRSIM_TOKEN_SET_RATIO || weighted_measure(measure);
    case STRSIM_ENTRY_BEST_MATCH: return reference_five;
    case STRSIM_ENTRY_CODEC: return reference_five;
    default: return false;
    }
}

} // namespace strsim

struct strsim_ctx;
extern "C" int strsim_internal_scan_workspace(strsim_ctx *ctx, uint32_t **p); // (hidden visibility: not exported)
extern "C" int strsim_internal_ctx_device(strsim_ctx *ctx);                   // the HIP device ordinal of a context
