// Host build of the cores of strsim_wratio.h, for tests/test_wratio_cpu.py: g++ compiles the same header; the test holds the class
// predicate and the rules to tests/wratio_ref.py and the row copy of the gather to memcpy at every alignment.
#include <stddef.h>
#include <stdint.h>

#include "strsim_wratio.h"

using namespace strsim;

extern "C" uint32_t wratio_class_c(uint32_t la, uint32_t lb) { return wratio_class(la, lb); }

extern "C" double wratio_rule_c(uint32_t cls, double r, double s0, double s1) { return wratio_rule(cls, r, s0, s1); }

extern "C" double partial_token_set_score_c(uint32_t sl, uint32_t la, uint32_t lb, uint32_t flags, double p)
{
    return partial_token_set_score(TokenSetRec{sl, la, lb, flags}, p);
}

// what the TAKE_LANES lanes of k_take_write do for one row, one lane after the other
extern "C" void take_copy_c(const uint8_t *src, uint8_t *dst, uint32_t len)
{
    for (uint32_t sub = 0; sub < TAKE_LANES; ++sub) take_copy(src, dst, len, sub);
}
