// Host build of the row functions of strsim_process.h, for tests/test_process_cpu.py: g++ compiles the same header, the test drives
// it row by row against tests/process_ref.py.  tier = 1 is what k_process_lane runs per lane (process_ascii_measure,
// process_ascii_write); tier = 0 is what k_process_wave runs per wave: the per-lane functions (process_decode, process_map,
// process_utf8_len, process_utf8_pack), the walk (process_walk_chunk) and the stores (process_put_word) are the header's, the
// ballots and the LDS words of the kernel are 64-element loops and an array here; tier = 2 is a textbook loop for comparison.
// Every row is copied to a heap block that ends with its last byte (a sanitizer sees a read behind it) at the source alignment
// asked for, and written into a block of guard bytes at the destination alignment asked for.
// With -DPROCESS_HARNESS_MAIN the file is a stand-alone program that sweeps lengths, alignments and contents (for ASan / UBSan).
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "strsim_process.h"

using namespace strsim;

static const ProcessTable T{PROCESS_BLOCK, PROCESS_CLASS, PROCESS_DELTA};
static const uint32_t NOT_LANE = 0xFFFFFFFFu, GUARD_HIT = 0xFFFFFFFEu;

static uint32_t popc(uint64_t v) { return (uint32_t)__builtin_popcountll((unsigned long long)v); }

// k_process_wave over one row; write = false returns the bytes, write = true fills dst[0, out_len)
static uint32_t wave_row(const uint8_t *p, uint32_t n, bool write, uint8_t *dst, uint32_t out_len)
{
    uint32_t s_w[32];
    memset(s_w, 0xEE, sizeof s_w);
    uint8_t *const s_b = reinterpret_cast<uint8_t *>(s_w);
    const uint32_t a = write ? (uint32_t)((uintptr_t)dst & 3u) : 0u;
    uint8_t *const base = dst - a;
    const uint32_t end = a + out_len;
    uint32_t v0 = a;
    ProcessWalk w{0u, 0u, 0u, false};
    for (uint32_t b0 = 0u; b0 < n; b0 += 64u) {
        bool st[64];
        uint32_t m[64], ol[64];
        uint64_t sm = 0, km = 0, m2 = 0, m3 = 0, m4 = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint32_t i = b0 + lane;
            st[lane] = i < n && (p[i] & 0xC0u) != 0x80u;
            m[lane] = 0x20u;
            ol[lane] = 0u;
            if (st[lane]) {
                m[lane] = process_map(process_decode(p, i, n), T);
                ol[lane] = process_utf8_len(m[lane]);
            }
            const uint64_t bit = 1ull << lane;
            if (st[lane]) sm |= bit;
            if (st[lane] && m[lane] != 0x20u) km |= bit;
            if (ol[lane] >= 2u) m2 |= bit;
            if (ol[lane] >= 3u) m3 |= bit;
            if (ol[lane] >= 4u) m4 |= bit;
        }
        const uint32_t cum0 = w.cum;
        process_walk_chunk(w, sm, km, popc(sm) + popc(m2) + popc(m3) + popc(m4));
        if (!write || !w.seen) continue;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint64_t below = (1ull << lane) - 1ull;
            const uint32_t at = cum0 + popc(sm & below) + popc(m2 & below) + popc(m3 & below) + popc(m4 & below);
            if (st[lane] && at >= w.lead && at - w.lead + ol[lane] <= out_len) {
                const uint32_t q = a + at - w.lead - (v0 & ~3u);
                if (q + ol[lane] > sizeof s_w) abort(); // (the kernel's LDS array)
                const uint32_t pk = process_utf8_pack(m[lane], ol[lane]);
                for (uint32_t k = 0; k < ol[lane]; ++k) s_b[q + k] = (uint8_t)(pk >> (8u * k));
            }
        }
        uint32_t e = w.cum - w.lead;
        e = e < out_len ? e : out_len;
        const uint32_t v1 = a + e, w0 = v0 >> 2, nw = (v1 >> 2) - w0;
        if (nw > 31u) abort();
        for (uint32_t lane = 0; lane < nw; ++lane) process_put_word(base, w0 + lane, s_w[lane], a, end);
        if (nw != 0u) s_w[0] = s_w[nw];
        v0 = v1;
    }
    if (!write) return process_walk_bytes(w);
    if ((v0 & 3u) != 0u) process_put_word(base, v0 >> 2, s_w[0], a, end);
    return out_len;
}

static std::vector<uint8_t> textbook(const uint8_t *p, uint32_t n)
{
    std::vector<uint32_t> cps;
    for (uint32_t i = 0; i < n; ++i)
        if ((p[i] & 0xC0u) != 0x80u) cps.push_back(process_map(process_decode(p, i, n), T));
    size_t lo = 0, hi = cps.size();
    while (lo < hi && cps[lo] == 0x20u) ++lo;
    while (hi > lo && cps[hi - 1] == 0x20u) --hi;
    std::vector<uint8_t> out;
    for (size_t k = lo; k < hi; ++k) {
        const uint32_t l = process_utf8_len(cps[k]), pk = process_utf8_pack(cps[k], l);
        for (uint32_t b = 0; b < l; ++b) out.push_back((uint8_t)(pk >> (8u * b)));
    }
    return out;
}

extern "C" uint32_t process_map_c(uint32_t cp) { return process_map(cp, T); }

extern "C" uint32_t process_lane_max_bytes_c(void) { return PROCESS_LANE_MAX_BYTES; }

extern "C" uint32_t process_map_ascii_word_c(uint32_t w) { return process_map_ascii_word(w); }

// The processed row of p[0, n) into out (n + n / 2 bytes suffice); returns its bytes, NOT_LANE when tier 1 does not take the row,
// GUARD_HIT when a byte outside the row's output was written.
extern "C" uint32_t process_row_c(const uint8_t *p, uint32_t n, int tier, uint32_t src_shift, uint32_t dst_shift, uint8_t *out)
{
    std::vector<uint8_t> tb;
    uint8_t *const src_block = static_cast<uint8_t *>(malloc(16u + src_shift + n)); // (malloc: 16-byte aligned)
    uint8_t *const src = src_block + 16u + src_shift;
    memset(src_block, 0x41, 16u + src_shift); // letters in front of the row: a read there would change the result
    if (n) memcpy(src, p, n);
    uint32_t bytes = 0u, first = 0u, hi = 0u;
    bool ok = true;
    if (tier == 1) {
        bytes = process_ascii_measure(src, n, first, hi);
        ok = n <= PROCESS_LANE_MAX_BYTES && (hi & 0x80808080u) == 0u;
    } else if (tier == 0) {
        bytes = wave_row(src, n, false, nullptr, 0u);
    } else {
        tb = textbook(src, n);
        bytes = (uint32_t)tb.size();
    }
    if (!ok) { free(src_block); return NOT_LANE; }
    const size_t guard = 16u, room = guard + dst_shift + bytes + guard;
    uint8_t *const dst_block = static_cast<uint8_t *>(malloc(room));
    memset(dst_block, 0xA5, room);
    uint8_t *const dst = dst_block + guard + dst_shift;
    if (tier == 1) process_ascii_write(src + first, dst, bytes);
    else if (tier == 0) wave_row(src, n, true, dst, bytes);
    else if (bytes) memcpy(dst, tb.data(), bytes);
    bool hit = false;
    for (size_t k = 0; k < room; ++k)
        if ((dst_block + k < dst || dst_block + k >= dst + bytes) && dst_block[k] != 0xA5) hit = true;
    if (bytes) memcpy(out, dst, bytes);
    free(dst_block);
    free(src_block);
    return hit ? GUARD_HIT : bytes;
}

#ifdef PROCESS_HARNESS_MAIN
// Lengths 0 .. 80 (and a few long rows) x every source and destination alignment x contents that include truncated sequences,
// stray continuation bytes, the growers and rows of nothing but lead bytes: both tiers against the textbook loop.
int main()
{
    static const char *const PIECES[] = {"a", "Z", " ", "_", ",", "9", "\xC8\xBA", "\xC8\xBE", "\xE2\x84\xAA", "\xC4\xB0", "\xF0\x90\x90\x80",
                                         "\xF0\x9F\x98\x80", "\xE3\x80\x80", "\xCC\x81", "\xE1\xBA\x9E", "\xC3", "\xE2\x84", "\xF0\x90\x90", "\x80", "\xFF"};
    const size_t NP = sizeof PIECES / sizeof PIECES[0];
    uint64_t seed = 12345u, rows = 0u;
    auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    std::vector<uint8_t> row, o0, o1, o2;
    for (uint32_t len = 0; len <= 84u; ++len) {
        const uint32_t target = len <= 80u ? len : 200u + 150u * (len - 80u);
        for (int kind = 0; kind < 12; ++kind) {
            row.clear();
            // kinds 6 .. 11: nothing but lead bytes, or lead bytes with too few continuation bytes -- every lane a start byte
            static const char *const DENSE[] = {"\xF0", "\xE4", "\xC8", "\xF8", "\xC8\xF0\xE4", "\xF0\x90\xE4\x80\xC8"};
            while (kind >= 6 && row.size() < target)
                for (const char *q = DENSE[kind - 6]; *q && row.size() < target; ++q) row.push_back((uint8_t)*q);
            while (row.size() < target) {
                const char *pc = kind == 0 ? PIECES[rnd() % 6u] : (kind == 1 ? " " : PIECES[rnd() % NP]);
                for (const char *q = pc; *q && row.size() < target; ++q) row.push_back((uint8_t)*q); // (the last piece may be cut: truncated)
            }
            o0.assign(target + target / 2u + 8u, 0);
            o1 = o0;
            o2 = o0;
            for (uint32_t sa = 0; sa < 4u; ++sa)
                for (uint32_t da = 0; da < 4u; ++da) {
                    const uint32_t n2 = process_row_c(row.data(), target, 2, sa, da, o2.data());
                    const uint32_t n0 = process_row_c(row.data(), target, 0, sa, da, o0.data());
                    const uint32_t n1 = process_row_c(row.data(), target, 1, sa, da, o1.data());
                    if (n2 > target + target / 2u) { printf("more than bytes + bytes / 2: len %u kind %d\n", target, kind); return 1; }
                    if (n0 != n2 || memcmp(o0.data(), o2.data(), n2) != 0) { printf("wave tier differs: len %u kind %d sa %u da %u\n", target, kind, sa, da); return 1; }
                    if (n1 != NOT_LANE && (n1 != n2 || memcmp(o1.data(), o2.data(), n2) != 0)) { printf("lane tier differs: len %u kind %d sa %u da %u\n", target, kind, sa, da); return 1; }
                    if (n1 == NOT_LANE && kind < 2 && target <= PROCESS_LANE_MAX_BYTES) { printf("lane tier refused an ASCII row: len %u\n", target); return 1; }
                    ++rows;
                }
        }
    }
    printf("process harness ok: %llu rows\n", (unsigned long long)rows);
    return 0;
}
#endif
