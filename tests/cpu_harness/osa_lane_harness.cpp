// Host build of the one-pair-per-lane OSA recurrence of strsim_osa.h (the code k_osa_lane runs per lane), for
// tests/test_osa_cpu.py: g++ compiles the same header, the test drives it pair by pair against tests/osa_ref.py.
#include <stdint.h>
#include <string.h>

#include "strsim_osa.h"

using namespace strsim;

static void window64(const char *s, uint32_t len, uint32_t (&w)[16])
{
    uint8_t b[64] = {};
    memcpy(b, s, len);
    for (int d = 0; d < 16; ++d) w[d] = (uint32_t)b[4 * d] | ((uint32_t)b[4 * d + 1] << 8) | ((uint32_t)b[4 * d + 2] << 16) | ((uint32_t)b[4 * d + 3] << 24);
}

// OSA distance of pattern p (lp <= 64 ASCII bytes) and text t (lt <= 64), with the 32-bit masks when wide == 0 (lp <= 32).
// tmax >= lt: the columns the wave runs (a longer text of another lane); the state must not move beyond lt.
extern "C" uint32_t osa_lane_distance(const char *p, uint32_t lp, const char *t, uint32_t lt, uint32_t tmax, int wide)
{
    uint32_t wp[16], wt[16], Plo[7], Phi[7];
    window64(p, lp, wp);
    window64(t, lt, wt);
    osa_planes(wp, Plo, Phi, wide != 0);
    return wide ? osa_lane_core<uint64_t>(wt, lt, tmax, Plo, Phi, lp) : osa_lane_core<uint32_t>(wt, lt, tmax, Plo, Phi, lp);
}

extern "C" double osa_lane_score(uint32_t d, uint32_t la, uint32_t lb) { return epilogue_osa(d, la, lb); }
