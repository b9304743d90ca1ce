// qgram_harness.cpp -- host replay of the q-gram kernels' shared code (strsim_qgram.h): the lane core (qgram_lane_pair, as
// k_qgram_lane runs it on zero-padded 64-byte windows, at either mask width) and the table rules of k_qgram_wave (qgram_key,
// qgram_table_slots, qgram_claim, qgram_tally) over a plain array, each against a brute force over std::map.
//
// Built by tests/test_qgram_cpu.py as a shared library (g++ -shared), and with -DQGRAM_HARNESS_MAIN as a stand-alone program that
// runs every sweep once and exits non-zero on a mismatch -- the form the sanitizers are run on.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "strsim_qgram.h"

using namespace strsim;

namespace {

using Gram = std::array<uint32_t, 3>;

std::map<Gram, uint32_t> brute_grams(const uint32_t *v, uint32_t n, uint32_t q)
{
    std::map<Gram, uint32_t> m;
    for (uint32_t i = 0; i + q <= n; ++i) {
        Gram g{0u, 0u, 0u};
        for (uint32_t k = 0; k < q; ++k) g[k] = v[i + k];
        ++m[g];
    }
    return m;
}

// -> I, na, nb
void brute(const uint32_t *a, uint32_t ca, const uint32_t *b, uint32_t cb, uint32_t q, bool set, uint32_t out[3])
{
    const auto ma = brute_grams(a, ca, q), mb = brute_grams(b, cb, q);
    uint32_t isect = 0, na = 0, nb = 0;
    for (const auto &e : ma) {
        na += set ? 1u : e.second;
        const auto f = mb.find(e.first);
        if (f != mb.end()) isect += set ? 1u : (e.second < f->second ? e.second : f->second);
    }
    for (const auto &e : mb) nb += set ? 1u : e.second;
    out[0] = isect; out[1] = na; out[2] = nb;
}

void window(const uint8_t *s, uint32_t len, uint32_t (&w)[16])
{
    uint8_t buf[64] = {};
    memcpy(buf, s, len);
    memcpy(w, buf, 64);
}

template <typename T>
QgramCounts lane_at(const uint32_t (&wa)[16], uint32_t la, const uint32_t (&wb)[16], uint32_t lb, uint32_t q, bool set, uint32_t amax, uint32_t bmax)
{
    if (q == 1) return set ? qgram_lane_pair<T, 1, true>(wa, la, amax, wb, lb, bmax) : qgram_lane_pair<T, 1, false>(wa, la, amax, wb, lb, bmax);
    if (q == 2) return set ? qgram_lane_pair<T, 2, true>(wa, la, amax, wb, lb, bmax) : qgram_lane_pair<T, 2, false>(wa, la, amax, wb, lb, bmax);
    return set ? qgram_lane_pair<T, 3, true>(wa, la, amax, wb, lb, bmax) : qgram_lane_pair<T, 3, false>(wa, la, amax, wb, lb, bmax);
}

uint64_t xorshift(uint64_t &s)
{
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return s;
}

} // namespace

extern "C" {

// The lane core on one pair of ASCII strings of up to 64 bytes.  words: 1 (both at most 32 bytes) or 2 mask words; slack: how far
// the wave's longest strings (amax, bmax) lie above this pair's, as in a wave of mixed lengths.  -> out = I, na, nb; 0, or -1 when
// the pair does not fit the width.
int qgram_lane(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb, uint32_t q, int set, int words, uint32_t slack, uint32_t *out)
{
    const uint32_t cap = words == 1 ? 32u : 64u;
    if (la > cap || lb > cap || q < 1 || q > 3) return -1;
    uint32_t wa[16], wb[16];
    window(a, la, wa);
    window(b, lb, wb);
    const uint32_t amax = la + slack < cap ? la + slack : cap, bmax = lb + slack < cap ? lb + slack : cap;
    const QgramCounts c = words == 1 ? lane_at<uint32_t>(wa, la, wb, lb, q, set != 0, amax, bmax) : lane_at<uint64_t>(wa, la, wb, lb, q, set != 0, amax, bmax);
    out[0] = c.isect; out[1] = c.na; out[2] = c.nb;
    return 0;
}

// Every length pair 0..64 x 0..64 of random strings over alphabet[0 .. nalpha) at (q, set), at each mask width that holds the pair
// and with the wave's longest text both equal to and above the pair's, against the brute force.  -> the number of mismatches;
// first[0..7] = la, lb, words, got I na nb's first disagreement with want (I, na, nb packed as got[3], want[3] behind la, lb).
uint64_t qgram_lane_sweep(const uint8_t *alphabet, uint32_t nalpha, uint64_t seed, uint32_t q, int set, uint32_t *first)
{
    uint64_t bad = 0, rng = seed * 0x9E3779B97F4A7C15ull + 1u;
    for (uint32_t la = 0; la <= 64; ++la)
        for (uint32_t lb = 0; lb <= 64; ++lb) {
            uint8_t a[64], b[64];
            uint32_t va[64], vb[64];
            for (uint32_t i = 0; i < la; ++i) va[i] = a[i] = alphabet[xorshift(rng) % nalpha];
            for (uint32_t i = 0; i < lb; ++i) vb[i] = b[i] = alphabet[xorshift(rng) % nalpha];
            uint32_t want[3];
            brute(va, la, vb, lb, q, set != 0, want);
            for (int words = 1; words <= 2; ++words)
                for (uint32_t slack = 0; slack <= 5; slack += 5) {
                    uint32_t got[3];
                    if (qgram_lane(a, la, b, lb, q, set, words, slack, got)) continue;
                    if (memcmp(got, want, sizeof got) != 0 && bad++ == 0 && first) {
                        first[0] = la; first[1] = lb; first[2] = (uint32_t)words;
                        memcpy(first + 3, got, sizeof got);
                        memcpy(first + 6, want, sizeof want);
                    }
                }
        }
    return bad;
}

// The table rules over a plain array: the grams of the scalar values va / vb claimed with qgram_claim (a compare-and-swap that is
// a plain compare and store) in a table of qgram_table_slots(ga + gb) slots, counted in a word of `count_bytes` (4 or 8) a slot and
// tallied.  -> out = I, na, nb, the slots, the longest probe sequence; 0, or -1 when a claim found no slot.
int qgram_table(const uint32_t *va, uint32_t ca, const uint32_t *vb, uint32_t cb, uint32_t q, int set, int count_bytes, uint64_t *out)
{
    const uint32_t ga = qgram_count(ca, q), gb = qgram_count(cb, q);
    const uint64_t slots = qgram_table_slots((uint64_t)ga + gb);
    const uint32_t mask = (uint32_t)slots - 1u;
    std::vector<uint64_t> keys(slots, QGRAM_EMPTY), cnt(slots, 0);
    uint64_t longest = 0;
    int rc = 0;
    auto cas = [&](uint64_t *p, uint64_t expected, uint64_t desired) {
        const uint64_t found = *p;
        if (found == expected) *p = desired;
        return found;
    };
    auto insert = [&](const uint32_t *v, uint32_t g, int side) {
        for (uint32_t i = 0; i < g; ++i) {
            const uint64_t key = qgram_key(v[i], q >= 2 ? v[i + 1] : 0u, q >= 3 ? v[i + 2] : 0u);
            const uint32_t s = qgram_claim(keys.data(), mask, key, cas);
            if (keys[s] != key) { rc = -1; continue; }
            const uint64_t dist = (s - qgram_hash(key, mask)) & mask;
            if (dist > longest) longest = dist;
            cnt[s] += count_bytes == 4 ? (uint64_t)qgram_count_one<uint32_t>(side) : qgram_count_one<uint64_t>(side);
        }
    };
    insert(va, ga, 0);
    insert(vb, gb, 1);
    uint32_t isect = 0, da = 0, db = 0;
    for (uint64_t s = 0; s < slots; ++s) {
        if (count_bytes == 4) {
            if (set) qgram_tally<uint32_t, true>((uint32_t)cnt[s], isect, da, db);
            else qgram_tally<uint32_t, false>((uint32_t)cnt[s], isect, da, db);
        } else {
            if (set) qgram_tally<uint64_t, true>(cnt[s], isect, da, db);
            else qgram_tally<uint64_t, false>(cnt[s], isect, da, db);
        }
    }
    out[0] = isect; out[1] = set ? da : ga; out[2] = set ? db : gb; out[3] = slots; out[4] = longest;
    return rc;
}

void qgram_brute(const uint32_t *va, uint32_t ca, const uint32_t *vb, uint32_t cb, uint32_t q, int set, uint32_t *out) { brute(va, ca, vb, cb, q, set != 0, out); }

double qgram_score_c(int kind, uint64_t isect, uint64_t na, uint64_t nb, int same) { return qgram_score(kind, isect, na, nb, same != 0); }

uint64_t qgram_key_c(uint32_t v0, uint32_t v1, uint32_t v2) { return qgram_key(v0, v1, v2); }
uint32_t qgram_hash_c(uint64_t key, uint32_t mask) { return qgram_hash(key, mask); }
uint64_t qgram_table_slots_c(uint64_t grams) { return qgram_table_slots(grams); }
uint64_t qgram_wave_slot_words_c(uint64_t grams, uint64_t values) { return qgram_wave_slot_words(grams, values); }

// Random scalar values over `nvalues` values spread to the 21-bit range (scale), both count widths, q = 1..3, both modes, lengths
// around the LDS limits; the keys that collide in the table's hash; the key nearest QGRAM_EMPTY.  -> mismatches
uint64_t qgram_table_sweep(uint64_t seed)
{
    uint64_t bad = 0, rng = seed * 0x9E3779B97F4A7C15ull + 7u;
    const uint32_t lens[] = {0, 1, 2, 3, 4, 31, 64, 65, 127, 128, 129, 255, 1024, 1025, 1500, 5000};
    const uint32_t alphas[] = {1, 2, 8, 0x10FFFFu};
    for (uint32_t nv : alphas)
        for (uint32_t ca : lens)
            for (uint32_t cb : {ca, ca / 2u + 1u, 3u}) {
                std::vector<uint32_t> va(ca + 1), vb(cb + 1);
                for (uint32_t i = 0; i < ca; ++i) va[i] = nv <= 8 ? (uint32_t)(xorshift(rng) % nv) * 0x3FFFFu : (uint32_t)(xorshift(rng) % 0x110000u);
                for (uint32_t i = 0; i < cb; ++i) vb[i] = nv <= 8 ? (uint32_t)(xorshift(rng) % nv) * 0x3FFFFu : va[xorshift(rng) % (ca ? ca : 1u)];
                for (uint32_t q = 1; q <= 3; ++q)
                    for (int set = 0; set <= 1; ++set)
                        for (int bytes = 4; bytes <= 8; bytes += 4) {
                            if (bytes == 4 && qgram_count(ca, q) + qgram_count(cb, q) > QGRAM_WAVE_LDS_GRAMS) continue; // (16-bit halves)
                            uint32_t want[3];
                            uint64_t got[5];
                            brute(va.data(), ca, vb.data(), cb, q, set != 0, want);
                            if (qgram_table(va.data(), ca, vb.data(), cb, q, set, bytes, got) != 0) ++bad;
                            else if (got[0] != want[0] || got[1] != want[1] || got[2] != want[2]) ++bad;
                            const uint64_t grams = (uint64_t)qgram_count(ca, q) + qgram_count(cb, q);
                            if (got[3] < 2 * grams || (got[3] & (got[3] - 1))) ++bad; // load <= 1/2, a power of two
                        }
            }
    // keys that share a home slot: found by search over the third value, at load exactly 1/2
    {
        const uint32_t n = 32; // 32 grams of a, the same of b: 64 grams, 128 slots
        const uint32_t mask = (uint32_t)qgram_table_slots(2 * n) - 1u;
        std::vector<uint32_t> va, vb;
        const uint32_t home = qgram_hash(qgram_key(5, 0, 0), mask);
        for (uint32_t v = 0; va.size() < n && v < 0x110000u; ++v)
            if (qgram_hash(qgram_key(v, 0, 0), mask) == home) va.push_back(v);
        vb.assign(va.rbegin(), va.rend());
        uint32_t want[3];
        uint64_t got[5];
        brute(va.data(), n, vb.data(), n, 1, false, want);
        if (va.size() != n || qgram_table(va.data(), n, vb.data(), n, 1, 0, 4, got) != 0 || got[0] != want[0] || got[0] != n || got[4] != n - 1) ++bad;
    }
    // the key nearest the empty value: three times the largest 21-bit value, next to grams that differ from it in one value
    {
        const uint32_t top = 0x1FFFFFu;
        const uint32_t va[] = {top, top, top, top, top - 1u, top, top}, vb[] = {top, top, top, 0u, top, top, top, top};
        for (uint32_t q = 1; q <= 3; ++q)
            for (int set = 0; set <= 1; ++set) {
                uint32_t want[3];
                uint64_t got[5];
                brute(va, 7, vb, 8, q, set != 0, want);
                if (qgram_table(va, 7, vb, 8, q, set, 8, got) != 0 || got[0] != want[0] || got[1] != want[1] || got[2] != want[2]) ++bad;
            }
        if (qgram_key(top, top, top) == QGRAM_EMPTY || (qgram_key(top, top, top) >> 63)) ++bad;
    }
    return bad;
}

} // extern "C"

#ifdef QGRAM_HARNESS_MAIN
int main()
{
    const uint8_t one[] = {'a'}, two[] = {'a', 'b'}, eight[] = {'a', 'b', 'c', 'd', 'e', 'f', 'g', 'h'};
    uint8_t bytes[128];
    for (int i = 0; i < 128; ++i) bytes[i] = (uint8_t)i; // every ASCII byte, NUL included
    const uint8_t nul[] = {0, 'a'};
    struct { const uint8_t *p; uint32_t n; const char *name; } alphabets[] = {{one, 1, "1 letter"}, {two, 2, "2 letters"}, {eight, 8, "8 letters"},
                                                                               {bytes, 128, "ASCII with NUL"}, {nul, 2, "NUL and a"}};
    uint64_t bad = 0, pairs = 0;
    for (const auto &al : alphabets)
        for (uint32_t q = 1; q <= 3; ++q)
            for (int set = 0; set <= 1; ++set) {
                uint32_t first[9] = {};
                const uint64_t b = qgram_lane_sweep(al.p, al.n, 17u + q, q, set, first);
                pairs += 65u * 65u;
                if (b) printf("lane sweep %s q=%u set=%d: %llu mismatches, first at la=%u lb=%u words=%u got %u %u %u want %u %u %u\n", al.name, q, set,
                              (unsigned long long)b, first[0], first[1], first[2], first[3], first[4], first[5], first[6], first[7], first[8]);
                bad += b;
            }
    const uint64_t tb = qgram_table_sweep(3);
    if (tb) printf("table sweep: %llu mismatches\n", (unsigned long long)tb);
    bad += tb;
    printf("qgram harness: %llu length pairs of the lane core, the table sweep: %llu mismatches\n", (unsigned long long)pairs, (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
