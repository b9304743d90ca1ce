// strsim_cdist.h -- cdist: the full score matrix of a query column against a candidate column (strsim_cdist_device, DESIGN.md
// section 20; rapidfuzz's process.cdist with scores / 100).  out[i * ld + j] is bit for bit the pairwise score of (queries[i],
// candidates[j]); under a cutoff a score below it is stored as 0.0.
//
// This header holds what the host shares with the kernel (tests/cpu_harness/cdist_harness.cpp compiles it with g++): the Indel
// score table, the candidate split, and the store schedule of a wave's tile -- which lane writes which (i, j) in which pass, at
// which 64-bit index, with which width.  The kernels are in strsim_cdist_kernels.h.
//
// The tile.  A wave of k_cdist_lane holds 64 queries, one per lane, and scores them against CDIST_TJ candidates in turn: lane l's
// score of the tile's candidate jj goes to s_tile[cdist_tile_at(l, jj)] (a column-wise write: 64 lanes, stride CDIST_STRIDE
// doubles).  The tile is then written out row-wise.  A row's segment is n <= CDIST_TJ contiguous doubles of `out`; whether its
// first double is 16-byte aligned depends on the row (base, i * ld and the tile's first candidate), so a row is cut into
// CDIST_SLOTS slots of two columns that start at column -h, h = the parity of the first double's index in 8-byte units: every
// slot that lies inside the segment is an aligned 16-byte store, and the one that straddles its head or its tail is an 8-byte
// store.  The 64 * CDIST_SLOTS items of a tile are dealt to the lanes row-major (item t = pass * 64 + lane: row t / CDIST_SLOTS,
// slot t % CDIST_SLOTS), so the lanes of one store instruction cover whole rows, 64 / CDIST_SLOTS of them.
//
// Banks (64 banks of 4 bytes; a store's bank is the dword address mod 32 within groups of 16 lanes, an 8-byte read's mod 64
// within 32 lanes).  CDIST_STRIDE = CDIST_TJ + 1 is odd: the 16 lanes of a write group are at dwords 2 * (l * STRIDE + jj),
// l * STRIDE mod 16 takes 16 values, so the column-wise writes do not conflict.  The row-wise reads are two 8-byte reads per item.
// At CDIST_TJ = 8 a read group of 32 lanes covers six and a half rows of five slots (4 dwords apart, 20 dwords a row); rows are
// 2 * STRIDE = 18 dwords apart, so rows r + 1 and r + 3 fall between the slots of row r (18 and 54 are 2 mod 4), row r + 2 lies
// beside it (36 .. 55) and only row r + 4 (72 = 8 mod 64) lands on its banks: 2-way on part of a group, ten reads per tile of
// 512 pairs.  No odd stride avoids it -- 32 lanes x 2 dwords fill the 64 banks exactly, and the fifth slot of the misaligned row
// makes a row's footprint 20 dwords, not 16.
//
// The sizes are chosen by measurement: CDIST_TJ = 8 and workgroups of CDIST_BLOCK = 512 threads, whose eight
// waves share one 33.8 KB score table beside eight tiles of 4.6 KB (70.7 KB of LDS: two workgroups, sixteen waves per CU, the
// occupancy of k_match_lane).  -DSTRSIM_CDIST_TJ / -DSTRSIM_CDIST_BLOCK build the other shapes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "strsim_indel.h"
#include "strsim_nearest.h"

namespace strsim {

#ifndef STRSIM_CDIST_TJ
#define STRSIM_CDIST_TJ 8
#endif
#ifndef STRSIM_CDIST_BLOCK
#define STRSIM_CDIST_BLOCK 512
#endif
constexpr uint32_t CDIST_TJ = STRSIM_CDIST_TJ;        // candidates per tile (8 or 16)
constexpr uint32_t CDIST_BLOCK = STRSIM_CDIST_BLOCK;  // threads of a workgroup of k_cdist_lane: its waves share one score table
constexpr uint32_t CDIST_STRIDE = CDIST_TJ + 1u;      // doubles per tile row
constexpr uint32_t CDIST_TILE = 64u * CDIST_STRIDE;   // doubles per wave
constexpr uint32_t CDIST_SLOTS = CDIST_TJ / 2u + 1u;  // two-column slots of a row, one more than fit: the misaligned row's tail
constexpr uint32_t CDIST_PASSES = CDIST_SLOTS;        // 64 * CDIST_SLOTS items, 64 per pass
static_assert(CDIST_TJ == 8u || CDIST_TJ == 16u, "a tile is 8 or 16 candidates wide");
static_assert(CDIST_BLOCK % 64u == 0u && CDIST_BLOCK >= 64u && CDIST_BLOCK <= 1024u, "a workgroup is 1 to 16 waves");

// The Indel score of a lane-class pair with distance d and length sum s: score[s * CDIST_TAB_W + d] = epilogue_indel(d, s, 0),
// d <= s <= 64 (0.0 where d > s: no such pair).  The same size as the quotient table of the reference measures.
constexpr uint32_t CDIST_TAB_W = 2u * NEAREST_MAX_LEN + 1u;
constexpr uint32_t CDIST_TAB_N = CDIST_TAB_W * CDIST_TAB_W;
inline void cdist_build_indel_table(double *score)
{
    for (uint32_t s = 0; s < CDIST_TAB_W; ++s)
        for (uint32_t d = 0; d < CDIST_TAB_W; ++d) score[s * CDIST_TAB_W + d] = d <= s ? epilogue_indel(d, s, 0u) : 0.0;
}

// The cutoff rule (rapidfuzz's): a score below the cutoff is stored as 0.0.  cutoff is not NaN; -inf and 0.0 change nothing.
STRSIM_HD double cdist_cut(double v, double cutoff) { return v < cutoff ? 0.0 : v; }

// out[i][j]
STRSIM_HD size_t cdist_index(uint64_t i, uint64_t ld, uint64_t j) { return (size_t)(i * ld + j); }

// Split s of `per` candidates each: [j0, j1).
STRSIM_HD void cdist_split_range(uint32_t s, uint32_t per, uint32_t nc, uint32_t &j0, uint32_t &j1)
{
    const uint64_t a = (uint64_t)s * per;
    j0 = a < nc ? (uint32_t)a : nc;
    j1 = nc - j0 < per ? nc : j0 + per;
}

// Candidate splits of k_cdist_lane for nq queries x nc candidates: about four workgroups per CU in all (two are resident), at
// least four tiles per split.  No list is written per split, so nothing else bounds the count.
inline uint32_t cdist_splits(uint64_t nq, uint64_t nc, int num_cu)
{
    const uint64_t qblocks = (nq + CDIST_BLOCK - 1u) / CDIST_BLOCK;
    const uint64_t target = 4u * (uint64_t)(num_cu > 0 ? num_cu : 256);
    uint64_t s = (target + qblocks - 1u) / (qblocks ? qblocks : 1u);
    const uint64_t by_tiles = (nc + 4u * CDIST_TJ - 1u) / (4u * CDIST_TJ);
    if (s > by_tiles) s = by_tiles;
    if (s > 65535u) s = 65535u;
    return s ? (uint32_t)s : 1u;
}

// Where lane l keeps its score of the tile's candidate jj.
STRSIM_HD uint32_t cdist_tile_at(uint32_t l, uint32_t jj) { return l * CDIST_STRIDE + jj; }

// Item t (0 .. 64 * CDIST_SLOTS - 1) of the write-out of a tile whose first row is query i0 (`rows` <= 64 of them exist) and
// whose n <= CDIST_TJ columns start at candidate jt; base8 is the address of `out` in 8-byte units.  The item stores `count`
// (0, 1 or 2) doubles of tile row `row` from column `col` on, at out[cdist_index(i0 + row, ld, jt + col)]; a count of 2 is
// 16-byte aligned.
struct CdistItem {
    uint32_t row, col, count;
};
STRSIM_HD CdistItem cdist_item(uint32_t t, uint64_t base8, uint32_t i0, uint32_t rows, uint64_t ld, uint32_t jt, uint32_t n)
{
    CdistItem it;
    it.row = t / CDIST_SLOTS;
    const uint32_t slot = t - it.row * CDIST_SLOTS;
    const uint32_t h = (uint32_t)((base8 + ((uint64_t)i0 + it.row) * ld + jt) & 1u);
    const uint32_t lo = 2u * slot > h ? 2u * slot - h : 0u; // the slot is columns [2 slot - h, 2 slot - h + 2), cut to [0, n)
    const uint32_t end = 2u * slot + 2u - h;
    const uint32_t hi = end < n ? end : n;
    it.col = lo;
    it.count = it.row < rows && hi > lo ? hi - lo : 0u;
    return it;
}

} // namespace strsim
