// common_harness.cpp -- host replay of the shared code of the Hamming / prefix / postfix kernels (strsim_common.h): the lane core
// as k_common_lane runs it (zero-padded 32-byte windows, the mask of differing bytes, the end alignment) and the three walks of
// k_common_wave over 64 emulated lanes (the byte prefix and suffix with their UTF-8 boundary rules, the lockstep walk with its two
// cursors and the 64-slot stages), each against brute force over decoded scalar values.  Every byte is read from a heap copy of
// exactly the string's size, so that a read outside the string is an error under AddressSanitizer.
//
// Built by tests/test_common_cpu.py as a shared library (g++ -shared), and with -DCOMMON_HARNESS_MAIN as a stand-alone program that
// runs every sweep and exits non-zero on a mismatch -- the form the sanitizers are run on.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "strsim_common.h"

using namespace strsim;

namespace {

typedef std::vector<uint8_t> Bytes;

bool is_start(const Bytes &p, uint32_t i) { return i < p.size() && (p[i] & 0xC0u) != 0x80u; }

// osa_decode_at of strsim_wave_util.h
uint32_t decode_at(const Bytes &p, uint32_t i)
{
    const uint32_t len = (uint32_t)p.size(), b0 = p[i];
    auto cont = [&](uint32_t k) { return i + k < len ? (uint32_t)(p[i + k] & 0x3Fu) : 0u; };
    if (b0 < 0x80u) return b0;
    if (b0 < 0xE0u) return ((b0 & 0x1Fu) << 6) | cont(1);
    if (b0 < 0xF0u) return ((b0 & 0x0Fu) << 12) | (cont(1) << 6) | cont(2);
    return ((b0 & 0x07u) << 18) | (cont(1) << 12) | (cont(2) << 6) | cont(3);
}

std::vector<uint32_t> decode(const Bytes &p)
{
    std::vector<uint32_t> v;
    for (uint32_t i = 0; i < p.size(); ++i)
        if (is_start(p, i)) v.push_back(decode_at(p, i));
    return v;
}

// brute force over scalar values
uint32_t brute(int kind, const Bytes &a, const Bytes &b)
{
    std::vector<uint32_t> x = decode(a), y = decode(b);
    if (kind == COMMON_POSTFIX) {
        std::reverse(x.begin(), x.end());
        std::reverse(y.begin(), y.end());
    }
    const size_t m = std::min(x.size(), y.size());
    uint32_t c = 0;
    for (size_t i = 0; i < m; ++i) {
        if (x[i] == y[i]) ++c;
        else if (kind != COMMON_HAMMING) break;
    }
    return c;
}

void window(const Bytes &s, uint32_t (&w)[8])
{
    uint8_t buf[32] = {};
    if (!s.empty()) memcpy(buf, s.data(), s.size());
    memcpy(w, buf, 32);
}

// k_common_lane's pair (both strings ASCII and <= COMMON_LANE_MAX bytes)
uint32_t lane(int kind, const Bytes &a, const Bytes &b)
{
    uint32_t wa[8], wb[8];
    window(a, wa);
    window(b, wb);
    const uint32_t la = (uint32_t)a.size(), lb = (uint32_t)b.size();
    if (kind == COMMON_PREFIX) return common_lane_count<COMMON_PREFIX>(wa, la, wb, lb);
    if (kind == COMMON_POSTFIX) return common_lane_count<COMMON_POSTFIX>(wa, la, wb, lb);
    return common_lane_count<COMMON_HAMMING>(wa, la, wb, lb);
}

// common_wave_prefix over 64 emulated lanes
uint32_t wave_prefix(const Bytes &a, const Bytes &b)
{
    const uint32_t na = (uint32_t)a.size(), nb = (uint32_t)b.size();
    uint32_t c = 0;
    for (uint32_t base = 0;; base += 64u) {
        uint64_t mm = 0, sa = 0, ka = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint32_t i = base + lane;
            const bool ina = i < na, inb = i < nb;
            const uint32_t xa = ina ? (uint32_t)a[i] : 0x100u, xb = inb ? (uint32_t)b[i] : 0x200u;
            mm |= (uint64_t)(xa != xb) << lane;
            sa |= (uint64_t)(ina && (xa & 0xC0u) != 0x80u) << lane;
            ka |= (uint64_t)(ina && (xa & 0xC0u) == 0x80u) << lane;
        }
        if (common_prefix_chunk(mm, sa, ka, c)) break;
    }
    return c;
}

uint32_t wave_suffix(const Bytes &a, const Bytes &b)
{
    const uint32_t na = (uint32_t)a.size(), nb = (uint32_t)b.size();
    uint32_t c = 0;
    for (uint32_t base = 0;; base += 64u) {
        uint64_t mm = 0, sa = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint32_t i = base + lane;
            const bool ina = i < na, inb = i < nb;
            const uint32_t xa = ina ? (uint32_t)a[na - 1u - i] : 0x100u, xb = inb ? (uint32_t)b[nb - 1u - i] : 0x200u;
            mm |= (uint64_t)(xa != xb) << lane;
            sa |= (uint64_t)(ina && (xa & 0xC0u) != 0x80u) << lane;
        }
        if (common_suffix_chunk(mm, sa, c)) break;
    }
    return c;
}

// common_wave_hamming over 64 emulated lanes; steps: how many steps it took
uint32_t wave_hamming(const Bytes &a, const Bytes &b, uint32_t *steps)
{
    const uint32_t na = (uint32_t)a.size(), nb = (uint32_t)b.size();
    uint32_t cura = 0, curb = 0, c = 0, n = 0;
    uint32_t s_a[64], s_b[64];
    for (;;) {
        uint64_t ma = 0, mb = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            ma |= (uint64_t)is_start(a, cura + lane) << lane;
            mb |= (uint64_t)is_start(b, curb + lane) << lane;
        }
        const CommonStep s = common_lockstep(ma, mb);
        if (s.t == 0u && (cura >= na || curb >= nb)) break;
        ++n;
        if (s.t != 0u) {
            for (uint32_t k = 0; k < 64u; ++k) s_a[k] = s_b[k] = 0xDEAD0000u + k;
            for (uint32_t lane = 0; lane < 64u; ++lane) {
                const uint32_t ra = osa_popc((uint64_t)(ma & common_low_ones64(lane))), rb = osa_popc((uint64_t)(mb & common_low_ones64(lane)));
                if (((ma >> lane) & 1u) && ra < s.t) s_a[ra] = decode_at(a, cura + lane);
                if (((mb >> lane) & 1u) && rb < s.t) s_b[rb] = decode_at(b, curb + lane);
            }
            for (uint32_t lane = 0; lane < s.t; ++lane) c += s_a[lane] == s_b[lane];
        }
        cura = common_advance(cura, s.t == 0u && ma != 0ull ? 0u : s.adva, na);
        curb = common_advance(curb, s.t == 0u && mb != 0ull ? 0u : s.advb, nb);
    }
    if (steps) *steps = n;
    return c;
}

uint32_t wave(int kind, const Bytes &a, const Bytes &b)
{
    if (kind == COMMON_PREFIX) return wave_prefix(a, b);
    if (kind == COMMON_POSTFIX) return wave_suffix(a, b);
    return wave_hamming(a, b, nullptr);
}

Bytes bytes_of(const std::string &s) { return Bytes(s.begin(), s.end()); }

int complain(const char *what, int kind, const Bytes &a, const Bytes &b, uint32_t got, uint32_t want)
{
    fprintf(stderr, "%s kind %d: got %u, want %u for (%.*s | %.*s)\n", what, kind, got, want, (int)a.size(), (const char *)a.data(), (int)b.size(),
            (const char *)b.data());
    return 1;
}

// both forms of a pair, both argument orders
int check_pair(int kind, const Bytes &a, const Bytes &b, bool lane_class)
{
    int bad = 0;
    const uint32_t want = brute(kind, a, b);
    if (lane_class) {
        if (lane(kind, a, b) != want) bad += complain("lane", kind, a, b, lane(kind, a, b), want);
        if (lane(kind, b, a) != want) bad += complain("lane", kind, b, a, lane(kind, b, a), want);
    }
    if (wave(kind, a, b) != want) bad += complain("wave", kind, a, b, wave(kind, a, b), want);
    if (wave(kind, b, a) != want) bad += complain("wave", kind, b, a, wave(kind, b, a), want);
    return bad;
}

// every length pair 0..33 over three letters, the first difference at every byte position -- from the front for prefix and
// Hamming, from the back for postfix -- and without any
int sweep_lengths()
{
    int bad = 0;
    std::mt19937 rng(7);
    const char abc[] = "abc";
    for (uint32_t la = 0; la <= 33u; ++la)
        for (uint32_t lb = 0; lb <= 33u; ++lb) {
            const uint32_t m = std::min(la, lb);
            for (uint32_t pos = 0; pos <= m; ++pos) { // pos == m: no difference inside the shorter string
                std::string lng(std::max(la, lb), 'a');
                for (auto &ch : lng) ch = abc[rng() % 3u];
                for (int kind = COMMON_HAMMING; kind <= COMMON_POSTFIX; ++kind) {
                    std::string a = lng.substr(kind == COMMON_POSTFIX ? lng.size() - la : 0u, la);
                    std::string b = lng.substr(kind == COMMON_POSTFIX ? lng.size() - lb : 0u, lb);
                    std::string &shorter = la <= lb ? a : b;
                    if (pos < m) {
                        const size_t at = kind == COMMON_POSTFIX ? m - 1u - pos : pos;
                        shorter[at] = shorter[at] == 'a' ? 'b' : 'a';
                        if (kind == COMMON_HAMMING) // more differences behind the first
                            for (size_t i = at + 1u; i < m; ++i)
                                if (rng() % 3u == 0u) shorter[i] = abc[rng() % 3u];
                    }
                    const Bytes x = bytes_of(a), y = bytes_of(b);
                    if (kind != COMMON_HAMMING && brute(kind, x, y) != pos) bad += complain("frame", kind, x, y, brute(kind, x, y), pos);
                    bad += check_pair(kind, x, y, la <= COMMON_LANE_MAX && lb <= COMMON_LANE_MAX);
                }
            }
        }
    return bad;
}

// n random lane pairs a kind: 0..32 bytes over 0x00..0x7F (NUL included), related by a few edits or a common head / tail
int sweep_lane_random(uint32_t n, uint32_t seed)
{
    int bad = 0;
    std::mt19937 rng(seed);
    for (int kind = COMMON_HAMMING; kind <= COMMON_POSTFIX; ++kind)
        for (uint32_t r = 0; r < n; ++r) {
            const uint32_t span = r % 4u == 0u ? 128u : 3u; // (a small alphabet makes long runs of equal bytes)
            Bytes a(rng() % 33u), b;
            for (auto &x : a) x = (uint8_t)(rng() % span);
            b = a;
            for (uint32_t e = rng() % 4u; e > 0u && !b.empty(); --e) b[rng() % b.size()] = (uint8_t)(rng() % span);
            const uint32_t how = rng() % 4u;
            if (how == 1u && !b.empty()) b.erase(b.begin(), b.begin() + rng() % b.size());
            if (how == 2u && !b.empty()) b.resize(rng() % b.size());
            if (how == 3u) {
                b.resize(rng() % 33u);
                for (auto &x : b) x = (uint8_t)(rng() % span);
            }
            bad += check_pair(kind, a, b, true);
        }
    return bad;
}

// the UTF-8 rules: all pairs of strings of up to 3 characters over a, e-acute, e-grave, copyright, euro, kip, U+10AC, a 4-byte one
// (C3 A9 / C3 A8 share a lead byte, C3 A9 / C2 A9 and E2 82 AC / E1 82 AC a tail, E2 82 AC / E2 82 AD two leading bytes)
int sweep_utf8()
{
    const char *alphabet[8] = {"a", "\xC3\xA9", "\xC3\xA8", "\xC2\xA9", "\xE2\x82\xAC", "\xE2\x82\xAD", "\xE1\x82\xAC", "\xF0\x9F\x98\x80"};
    std::vector<Bytes> words;
    words.push_back(Bytes());
    for (size_t from = 0, n = 0; n < 3; ++n) {
        const size_t to = words.size();
        for (size_t w = from; w < to; ++w)
            for (const char *ch : alphabet) {
                Bytes x = words[w];
                x.insert(x.end(), ch, ch + strlen(ch));
                words.push_back(x);
            }
        from = to;
    }
    int bad = 0;
    if (words.size() != 585u) bad += 1;
    for (const Bytes &a : words)
        for (const Bytes &b : words)
            for (int kind = COMMON_HAMMING; kind <= COMMON_POSTFIX; ++kind) {
                const uint32_t want = brute(kind, a, b), got = wave(kind, a, b);
                if (got != want) bad += complain("utf8", kind, a, b, got, want);
            }
    return bad;
}

// the lockstep walk (and the byte walks) on random mixed-width strings of lo..hi characters: one string over a 1- or 2-byte
// alphabet against an edited copy over another width, so that the cursors drift apart by more than a chunk
int sweep_lockstep(uint32_t n, uint32_t lo, uint32_t hi, uint32_t seed)
{
    const char *chars[8] = {"a", "b", "\xC3\xA9", "\xD0\xB1", "\xE2\x82\xAC", "\xE6\x97\xA5", "\xF0\x9F\x98\x80", "\xF0\x9D\x84\x9E"};
    std::mt19937 rng(seed);
    int bad = 0;
    uint32_t most = 0;
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t len = lo + rng() % (hi - lo + 1u);
        std::vector<uint32_t> x(len), y;
        const uint32_t wa = r % 3u == 0u ? 2u : 8u; // (a third: a one-byte string ...)
        for (auto &v : x) v = rng() % wa;
        y = x;
        if (r % 3u == 0u)
            for (auto &v : y) v = v + 6u; // (... against a four-byte one: 64 bytes hold 64 characters of one and 16 of the other)
        for (uint32_t e = rng() % 6u; e > 0u; --e) y[rng() % y.size()] = rng() % 8u;
        if (rng() % 2u) y.resize(lo / 2u + rng() % len);
        else if (rng() % 2u) y.erase(y.begin(), y.begin() + rng() % (len / 2u));
        Bytes a, b;
        for (uint32_t v : x) a.insert(a.end(), chars[v], chars[v] + strlen(chars[v]));
        for (uint32_t v : y) b.insert(b.end(), chars[v % 8u], chars[v % 8u] + strlen(chars[v % 8u]));
        for (int kind = COMMON_HAMMING; kind <= COMMON_POSTFIX; ++kind) bad += check_pair(kind, a, b, false);
        uint32_t steps = 0;
        wave_hamming(a, b, &steps);
        most = std::max(most, steps);
    }
    if (most < 3u) bad += 1; // (the frame must make the walk take several steps)
    return bad;
}

// the pieces on their own: the shifter against a byte copy, the n-th set bit against a loop
int sweep_pieces()
{
    int bad = 0;
    std::mt19937 rng(3);
    for (uint32_t delta = 0; delta <= 32u; ++delta) {
        uint8_t buf[32], want[32] = {};
        for (auto &x : buf) x = (uint8_t)(1u + rng() % 127u);
        memcpy(want, buf + delta, 32u - delta);
        uint32_t w[8];
        memcpy(w, buf, 32);
        common_shift_down(w, delta);
        if (memcmp(w, want, 32) != 0) { fprintf(stderr, "shift_down(%u)\n", delta); ++bad; }
    }
    for (uint32_t r = 0; r < 2000u; ++r) {
        uint64_t mask = ((uint64_t)rng() << 32) | rng();
        if (r % 4u == 1u) mask &= ((uint64_t)rng() << 32) | rng();
        if (r == 0u) mask = ~0ull;
        if (r == 2u) mask = 1ull << 63;
        uint32_t t = 0;
        for (uint32_t pos = 0; pos < 64u; ++pos)
            if ((mask >> pos) & 1ull) {
                if (common_nth_set(mask, t) != pos) { fprintf(stderr, "nth_set(%llx, %u)\n", (unsigned long long)mask, t); ++bad; }
                ++t;
            }
    }
    return bad;
}

} // namespace

extern "C" {
uint32_t common_lane_max_c() { return COMMON_LANE_MAX; }
uint32_t common_lane_c(int kind, const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb) { return lane(kind, Bytes(a, a + la), Bytes(b, b + lb)); }
uint32_t common_wave_c(int kind, const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb) { return wave(kind, Bytes(a, a + la), Bytes(b, b + lb)); }
uint32_t common_lane_row_c(int live, uint32_t la, uint32_t lb, int ascii, uint32_t k) { return common_lane_row(live != 0, la, lb, ascii != 0, k); }
uint64_t common_distance_c(uint64_t c, uint64_t la, uint64_t lb) { return common_distance(c, la, lb); }
uint32_t common_clamp_c(uint64_t d, uint32_t k) { return dist_clamp(d, k); }
double common_score_c(uint64_t c, uint64_t la, uint64_t lb) { return epilogue_osa(common_distance(c, la, lb), la, lb); }
int common_sweep_lengths_c() { return sweep_lengths(); }
int common_sweep_lane_random_c(uint32_t n, uint32_t seed) { return sweep_lane_random(n, seed); }
int common_sweep_utf8_c() { return sweep_utf8(); }
int common_sweep_lockstep_c(uint32_t n, uint32_t lo, uint32_t hi, uint32_t seed) { return sweep_lockstep(n, lo, hi, seed); }
int common_sweep_pieces_c() { return sweep_pieces(); }
}

#ifdef COMMON_HARNESS_MAIN
int main()
{
    int bad = 0;
    bad += sweep_pieces();
    bad += sweep_lengths();
    bad += sweep_lane_random(3000u, 11u);
    bad += sweep_utf8();
    bad += sweep_lockstep(400u, 60u, 140u, 5u);
    printf("common_harness: %d mismatches\n", bad);
    return bad != 0;
}
#endif
