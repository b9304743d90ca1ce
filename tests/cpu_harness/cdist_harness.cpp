// cdist_harness.cpp -- host build of the rules strsim_cdist.h shares with k_cdist_lane: the store schedule of a wave's tile
// replayed over a plain array with guard words around every row, the 64-bit index, the split rule and the Indel score table.
// Built by tests/test_cdist_cpu.py with g++ as a shared library; with -DCDIST_HARNESS_MAIN it is a stand-alone program that runs
// the whole sweep of shapes (the form that is run under the address and undefined-behaviour sanitizers).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "strsim_cdist.h"

using namespace strsim;

static const uint64_t GUARD_BITS = 0x7FF8DEADBEEF0001ull; // a NaN payload no score has
static const size_t EDGE = 4;                             // guard doubles in front of the first row and behind the last

static double value_of(uint32_t i, uint32_t j) { return (double)i * 4096.0 + (double)j + 0.5; }

// Replays k_cdist_lane's candidate loop and write-out for q queries x c candidates, leading dimension c + pad, the base 16-byte
// aligned (misalign = 0) or 8 bytes past it (1), `splits` candidate splits asked for.  0: every (i, j) was written exactly once
// with its own value, every 16-byte store was aligned and no guard was touched; otherwise the number of the first check that
// failed.
extern "C" int cdist_replay(uint32_t q, uint32_t c, uint32_t pad, uint32_t misalign, uint32_t splits)
{
    const size_t ld = (size_t)c + pad;
    const size_t total = 2 * EDGE + (size_t)q * ld + 2;
    double *const raw = static_cast<double *>(aligned_alloc(16, (total * sizeof(double) + 15) / 16 * 16));
    if (!raw) return 100;
    std::vector<uint8_t> hits(total, 0);
    double guard;
    memcpy(&guard, &GUARD_BITS, 8);
    for (size_t x = 0; x < total; ++x) raw[x] = guard;
    double *const out = raw + EDGE + misalign; // EDGE is even: raw + EDGE is 16-byte aligned
    const uint64_t base8 = (uint64_t)(uintptr_t)out >> 3;
    int bad = 0;
    if (q && c) {
        const uint32_t per = (c + splits - 1) / splits, nsplit = (c + per - 1) / per;
        std::vector<double> tile(CDIST_TILE);
        std::vector<uint8_t> filled(CDIST_TILE);
        for (uint32_t i0 = 0; i0 < q && !bad; i0 += 64) { // a wave
            const uint32_t rows = q - i0 < 64u ? q - i0 : 64u;
            for (uint32_t s = 0; s < nsplit && !bad; ++s) {
                uint32_t j0, j1;
                cdist_split_range(s, per, c, j0, j1);
                for (uint32_t jt = j0; jt < j1 && !bad; jt += CDIST_TJ) {
                    const uint32_t n = j1 - jt < CDIST_TJ ? j1 - jt : CDIST_TJ;
                    std::fill(filled.begin(), filled.end(), 0);
                    for (uint32_t jj = 0; jj < n; ++jj)
                        for (uint32_t l = 0; l < 64; ++l) { // the column-wise writes: every lane, live or not
                            const uint32_t at = cdist_tile_at(l, jj);
                            if (at >= CDIST_TILE || filled[at]) { bad = 1; break; }
                            filled[at] = 1;
                            tile[at] = value_of(i0 + l, jt + jj);
                        }
                    for (uint32_t t = 0; t < 64 * CDIST_PASSES && !bad; ++t) {
                        const CdistItem it = cdist_item(t, base8, i0, rows, ld, jt, n);
                        if (it.count > 2) { bad = 2; break; }
                        if (!it.count) continue;
                        if (it.row >= rows || it.col + it.count > n) { bad = 3; break; }
                        const size_t at = cdist_index((uint64_t)i0 + it.row, ld, (uint64_t)jt + it.col);
                        double *const dst = out + at;
                        if (it.count == 2 && ((uintptr_t)dst & 15u)) { bad = 4; break; }
                        for (uint32_t x = 0; x < it.count; ++x) {
                            const uint32_t src = cdist_tile_at(it.row, it.col + x);
                            if (!filled[src]) { bad = 5; break; }
                            dst[x] = tile[src];
                            if (++hits[(size_t)(dst + x - raw)] > 1) { bad = 6; break; }
                        }
                    }
                }
            }
        }
    }
    for (size_t x = 0; x < total && !bad; ++x) {
        const ptrdiff_t rel = (ptrdiff_t)x - (ptrdiff_t)(EDGE + misalign);
        const bool inside = rel >= 0 && (size_t)rel < (size_t)q * ld && c && (size_t)rel % ld < c;
        uint64_t bits;
        memcpy(&bits, &raw[x], 8);
        if (inside) {
            const uint32_t i = (uint32_t)((size_t)rel / ld), j = (uint32_t)((size_t)rel % ld);
            if (hits[x] != 1) bad = 7;
            else if (raw[x] != value_of(i, j)) bad = 8;
        } else if (hits[x] || bits != GUARD_BITS) bad = 9;
    }
    free(raw);
    return bad;
}

extern "C" uint64_t cdist_index_h(uint64_t i, uint64_t ld, uint64_t j) { return (uint64_t)cdist_index(i, ld, j); }

// item t of a tile at (i0, jt) -> row | col << 8 | count << 16
extern "C" uint32_t cdist_item_h(uint32_t t, uint64_t base8, uint32_t i0, uint32_t rows, uint64_t ld, uint32_t jt, uint32_t n)
{
    const CdistItem it = cdist_item(t, base8, i0, rows, ld, jt, n);
    return it.row | it.col << 8 | it.count << 16;
}

extern "C" uint32_t cdist_splits_h(uint64_t nq, uint64_t nc, int num_cu) { return cdist_splits(nq, nc, num_cu); }
extern "C" uint32_t cdist_tj(void) { return CDIST_TJ; }
extern "C" uint32_t cdist_block(void) { return CDIST_BLOCK; }

extern "C" double cdist_table_score(uint32_t d, uint32_t s)
{
    static double tab[CDIST_TAB_N];
    static bool ready = false;
    if (!ready) { cdist_build_indel_table(tab); ready = true; }
    return tab[s * CDIST_TAB_W + d];
}
extern "C" double cdist_epilogue(uint32_t d, uint32_t s) { return epilogue_indel(d, s, 0u); }
extern "C" double cdist_cut_h(double v, double cutoff) { return cdist_cut(v, cutoff); }

// Every shape of the sweep; the count of failures.
extern "C" uint32_t cdist_replay_all(void)
{
    static const uint32_t pads[3] = {0u, 1u, 3u};
    uint32_t failed = 0;
    for (uint32_t q = 0; q <= 130; ++q)
        for (uint32_t c = 0; c <= 40; ++c)
            for (uint32_t p = 0; p < 3; ++p)
                for (uint32_t m = 0; m < 2; ++m)
                    for (uint32_t s = 1; s <= 4; ++s)
                        if (cdist_replay(q, c, pads[p], m, s)) ++failed;
    return failed;
}

#ifdef CDIST_HARNESS_MAIN
int main()
{
    const uint32_t failed = cdist_replay_all();
    uint32_t table_bad = 0;
    for (uint32_t s = 0; s <= 64; ++s)
        for (uint32_t d = 0; d <= s; ++d)
            if (cdist_table_score(d, s) != cdist_epilogue(d, s)) ++table_bad;
    const uint64_t big = 0xFFFFFFFEull;
    const bool index_ok = cdist_index_h(big, big, big - 1) == big * big + big - 1;
    printf("cdist harness: %u shapes failed, %u table entries differ, 64-bit index %s\n", failed, table_bad, index_ok ? "exact" : "WRONG");
    return failed || table_bad || !index_ok ? 1 : 0;
}
#endif
