// strsim_components.h -- connected components of a CSR graph: one label per row (strsim_components_device, DESIGN.md section 23;
// the last stage of deduplication: "these 7 spellings are the same customer" is a component of the hit graph of a self-join).
//
// This header holds what the host shares with the kernels (tests/cpu_harness/components_harness.cpp compiles it with g++ over an
// accessor of std::atomic words): the row search of an edge, the hook-to-smaller rule of the link and the walk of the compress.
// The kernels are in strsim_components_kernels.h.
//
// The nnz edges (i, index[e]), e in [indptr[i], indptr[i + 1]), are read as undirected; duplicates and self-loops are harmless.
// parent[] is a forest with parent[x] <= x throughout:
//   - init      parent[v] = v;
//   - link      one lane per EDGE (a grid-stride loop bounded by nnz; the row of edge e by binary search of indptr), each hooks the
//               larger of the two roots it finds under the smaller (components_link);
//   - compress  a later launch: out_root[v] = the fixed point of parent from v -- once every edge is linked a component is one
//               tree, and its root is its smallest row, because parents never exceed their children;
//   - rank      flag[v] = (out_root[v] == v), its scan, out_cluster[v] = roots below out_root[v], the total is the count.
//
// Termination of a link (no lane waits for another, no workgroup for a workgroup).  Only a root is ever written (the CAS expects
// parent[hi] == hi) and only with a smaller value, so parent[x] <= x holds throughout and an entry that is not a root never changes
// again.  A step that neither finds hi under lo nor hooks it has read parent[hi] < hi -- or lost the CAS to a writer that made it
// so -- and goes on from parent[parent[hi]] <= parent[hi] < hi and parent[lo] <= lo < hi: the larger of the two values falls with
// every step, it starts at most at rows - 1 and a step needs it at least 1, so a link takes fewer than `rows` steps whatever the
// other lanes do.  Both values stay ancestors of the edge's two ends, so the link ends with the two ends in one tree.
//
// Memory safety, whatever indptr and index hold.  indptr is ASSUMED non-decreasing from 0 to nnz; nothing relies on it for an
// address.  components_edge_row searches words 1 .. rows of the rows + 1 words and returns a row below `rows`; an edge number e is
// below nnz, so index[e] is inside the caller's nnz words; an index[e] >= rows is never used as an address: the edge is skipped and
// counted in a device word that the call reads back with the count (STRSIM_ERR_ARG, "index out of range").  parent[], out_root[]
// and the scan are addressed by rows below `rows` only: by u, v < rows, and by values read from parent[], which are rows.  A wrong
// indptr therefore gives wrong labels, never an access outside the caller's buffers.
#pragma once
#include <stdint.h>

#include "strsim_join.h"

namespace strsim {

constexpr uint32_t COMPONENTS_BLOCK = 256u;    // threads of a workgroup of every components kernel
constexpr uint32_t COMPONENTS_MAX_GRID = 8192u; // workgroups of the link at most (a grid-stride loop over the edges)

// The row of edge e < nnz: the smallest r < rows with indptr[r + 1] > e (rows - 1 when there is none: a wrong indptr).  Reads
// words 1 .. rows only.  rows >= 1.
STRSIM_HD uint32_t components_edge_row(const uint64_t *indptr, uint32_t rows, uint64_t e)
{
    uint32_t lo = 0u, hi = rows - 1u; // the answer is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u; // < hi <= rows - 1
        if (indptr[(uint64_t)mid + 1u] > e) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// The hook-to-smaller rule for edge (u, v), both < rows, over an accessor of parent[]: load(x) and cas(x, expected, desired) ->
// the value found.  Returns the number of steps (< rows: see the top).
template <class Parent>
STRSIM_HD uint32_t components_link(Parent &parent, uint32_t u, uint32_t v)
{
    uint32_t p1 = parent.load(u), p2 = parent.load(v), steps = 0u;
    while (p1 != p2) {
        ++steps;
        const uint32_t hi = p1 > p2 ? p1 : p2, lo = p1 > p2 ? p2 : p1;
        const uint32_t ph = parent.load(hi);
        if (ph == lo) break;
        if (ph == hi && parent.cas(hi, hi, lo) == hi) break;
        p1 = parent.load(parent.load(hi));
        p2 = parent.load(lo);
    }
    return steps;
}

// The root of v: the fixed point of parent from v.  Read-only.
template <class Parent>
STRSIM_HD uint32_t components_find(const Parent &parent, uint32_t v)
{
    uint32_t p = parent.load(v);
    while (p != v) {
        v = p;
        p = parent.load(v);
    }
    return v;
}

// The workgroups of the link for nnz edges.
STRSIM_HD uint32_t components_link_grid(uint64_t nnz)
{
    const uint64_t b = (nnz + COMPONENTS_BLOCK - 1u) / COMPONENTS_BLOCK;
    return b > COMPONENTS_MAX_GRID ? COMPONENTS_MAX_GRID : (uint32_t)b;
}

} // namespace strsim
