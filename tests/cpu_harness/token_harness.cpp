// Host build of the tokenise / compare / sort / merge cores of strsim_token.h, for tests/test_token_cpu.py: g++ compiles the same
// header, the test drives it string by string against tests/token_ref.py.  lane = 1 is what k_token_*_lane runs per lane
// (token_split, insertion sort), lane = 0 what k_token_*_wave runs per wave (a token start per byte, the sorting network without
// stored padding); join, merge and score are the same code in both.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "strsim_token.h"

using namespace strsim;

static uint32_t split_sorted(const uint8_t *p, uint32_t n, TokenPairStore &d, uint32_t base, int lane)
{
    uint32_t cnt = 0;
    if (lane) {
        uint32_t hi = 0;
        cnt = token_split(p, n, d, base, 0xFFFFFFFFu, hi);
        token_isort(p, d, base, cnt);
    } else {
        for (uint32_t i = 0; i < n; ++i)
            if (token_is_start(p, i, n)) d.set(base + cnt++, i, token_end(p, i, n) - i);
        token_net_sort(p, d, base, cnt, 0u, 1u, [] {});
    }
    return cnt;
}

// join(sorted(tokens(p[0, n)))) into out (n bytes suffice); returns its bytes
extern "C" uint32_t token_sort_c(const uint8_t *p, uint32_t n, uint8_t *out, int lane)
{
    std::vector<uint32_t> desc(2 * (size_t)token_max_tokens(n) + 2);
    TokenPairStore d{desc.data()};
    const uint32_t cnt = split_sorted(p, n, d, 0u, lane);
    TokenSerialWriter w{out};
    return token_join(p, d, 0u, cnt, w);
}

// the set form of one pair: ab into out_ab (na bytes suffice), ba into out_ba; res = sl, la, lb, flags, bytes of ab, bytes of ba
extern "C" void token_set_c(const uint8_t *pa, uint32_t na, const uint8_t *pb, uint32_t nb, uint8_t *out_ab, uint8_t *out_ba, uint32_t *res,
                            int lane)
{
    std::vector<uint32_t> desc(2 * (size_t)(token_max_tokens(na) + token_max_tokens(nb)) + 2);
    TokenPairStore d{desc.data()};
    const uint32_t ca = split_sorted(pa, na, d, 0u, lane);
    const uint32_t cb = split_sorted(pb, nb, d, ca, lane);
    TokenSerialWriter wa{out_ab}, wb{out_ba};
    const TokenSetRec r = token_set_merge(pa, pb, d, 0u, ca, ca, cb, wa, wb, res[4], res[5]);
    res[0] = r.sl; res[1] = r.la; res[2] = r.lb; res[3] = r.flags;
}

extern "C" double token_set_score_c(uint32_t sl, uint32_t la, uint32_t lb, uint32_t flags, uint32_t d)
{
    return token_set_score(TokenSetRec{sl, la, lb, flags}, d);
}

extern "C" uint32_t token_space_len_c(const uint8_t *p, uint32_t i, uint32_t n) { return token_space_len(p, i, n); }
