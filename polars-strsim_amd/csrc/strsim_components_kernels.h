// strsim_components_kernels.h -- the kernels of strsim_components_device (the rules and their arguments are in strsim_components.h).
//   k_components_identity  nnz == 0: out_root[v] = out_cluster[v] = v.
//   k_components_init      parent[v] = v; thread 0 clears the two status words (count, bad indices).
//   k_components_link      one lane per edge, grid-stride over [0, nnz): components_link over relaxed agent-scope atomics (loads that
//                          bypass the CU's L1, so a lane sees what another CU's CAS wrote: the step count of the rule needs it).
//   k_components_compress  a launch of its own behind the link: out_root[v] = components_find, flag[v] = (out_root[v] == v) as the
//                          64-bit word the join's scan (k_join_scan_*) turns into the inclusive count of roots up to v.
//   k_components_rank      out_cluster[v] = scan[out_root[v]] - 1 (the roots below it); thread 0 stores the count, scan[rows - 1].
// No LDS beyond the scan's, no scratch, vector atomics only.
// Included by strsim_kernels.hip inside namespace strsim, after strsim_join_kernels.h (the scan is the join's).
#pragma once

struct ComponentsParentDevice {
    uint32_t *p;
    __device__ __forceinline__ uint32_t load(uint32_t x) const { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t cas(uint32_t x, uint32_t expected, uint32_t desired) { return atomicCAS(p + x, expected, desired); }
};

// parent[] as the launches behind the link read it: plain loads.
struct ComponentsParentPlain {
    const uint32_t *p;
    __device__ __forceinline__ uint32_t load(uint32_t x) const { return p[x]; }
};

__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_identity(uint32_t rows, uint32_t *__restrict__ out_root,
                                                                           uint32_t *__restrict__ out_cluster)
{
    const uint64_t v = (uint64_t)blockIdx.x * COMPONENTS_BLOCK + threadIdx.x;
    if (v >= rows) return;
    out_root[v] = (uint32_t)v;
    if (out_cluster) out_cluster[v] = (uint32_t)v;
}

__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_init(uint32_t rows, uint32_t *__restrict__ parent, uint64_t *__restrict__ status)
{
    const uint64_t v = (uint64_t)blockIdx.x * COMPONENTS_BLOCK + threadIdx.x;
    if (v == 0u) { status[0] = 0u; status[1] = 0u; }
    if (v < rows) parent[v] = (uint32_t)v;
}

__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_link(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ index,
                                                                       uint32_t rows, uint64_t nnz, uint32_t *parent, uint64_t *status)
{
    ComponentsParentDevice par{parent};
    uint32_t bad = 0u;
    const uint64_t stride = (uint64_t)gridDim.x * COMPONENTS_BLOCK;
    for (uint64_t e = (uint64_t)blockIdx.x * COMPONENTS_BLOCK + threadIdx.x; e < nnz; e += stride) {
        const uint32_t v = index[e];
        if (v >= rows) { ++bad; continue; }
        const uint32_t u = components_edge_row(indptr, rows, e);
        if (u != v) components_link(par, u, v);
    }
    if (bad) atomicAdd((unsigned long long *)(status + 1), (unsigned long long)bad);
}

__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_compress(uint32_t rows, const uint32_t *__restrict__ parent,
                                                                           uint32_t *__restrict__ out_root, uint64_t *__restrict__ flag)
{
    const uint64_t v = (uint64_t)blockIdx.x * COMPONENTS_BLOCK + threadIdx.x;
    if (v >= rows) return;
    const uint32_t r = components_find(ComponentsParentPlain{parent}, (uint32_t)v);
    out_root[v] = r;
    flag[v] = r == (uint32_t)v ? 1u : 0u;
}

__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_rank(uint32_t rows, const uint32_t *__restrict__ out_root,
                                                                       const uint64_t *__restrict__ scan, uint32_t *__restrict__ out_cluster,
                                                                       uint64_t *__restrict__ status)
{
    const uint64_t v = (uint64_t)blockIdx.x * COMPONENTS_BLOCK + threadIdx.x;
    if (v >= rows) return;
    if (v == 0u) status[0] = scan[(uint64_t)rows - 1u];
    if (out_cluster) out_cluster[v] = (uint32_t)(scan[out_root[v]] - 1u); // (a root's own flag is in its inclusive count)
}
