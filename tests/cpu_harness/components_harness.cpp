// components_harness.cpp -- host build of the rules strsim_components.h shares with the kernels of strsim_components_kernels.h,
// for tests/test_cluster_cpu.py: g++ compiles the same header over an accessor of std::atomic words.
//   ch_small        every edge order of every graph on 1 .. 5 vertices, linked sequentially (components_link), compressed
//                   (components_find) and ranked as the kernels do, against brute-force reachability; the steps of every link <= rows.
//   ch_threads      a random graph (every edge twice, in both orientations, self-loops and duplicates among them) linked by
//                   `threads` std::threads, edge e taken by thread e % threads, against a sequential union-find: roots, dense ids and
//                   count; guard words around parent[] and both outputs; the steps of every link <= rows.
//   ch_row_search   components_edge_row over indptr arrays with empty rows at the front, in the middle and at the end, every edge.
// Built as a shared library; with -DCOMPONENTS_HARNESS_MAIN it is a stand-alone program that runs every case (the form that is run
// under the address / undefined-behaviour and the thread sanitizers).
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <numeric>
#include <thread>
#include <vector>

#include "strsim_components.h"

using namespace strsim;

namespace {

const uint32_t GUARD = 0xDEADBEEFu;
const size_t EDGE = 8;

struct AtomicParent {
    std::atomic<uint32_t> *p;
    uint32_t load(uint32_t x) const { return p[x].load(std::memory_order_relaxed); }
    uint32_t cas(uint32_t x, uint32_t expected, uint32_t desired)
    {
        p[x].compare_exchange_strong(expected, desired, std::memory_order_relaxed);
        return expected; // (the value found)
    }
};

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0u; }
};

// compress and rank as k_components_compress / the scan / k_components_rank do; -> count
uint32_t labels(const AtomicParent &par, uint32_t rows, uint32_t *root, uint32_t *cluster)
{
    std::vector<uint64_t> scan(rows);
    for (uint32_t v = 0; v < rows; ++v) {
        root[v] = components_find(par, v);
        scan[v] = root[v] == v ? 1u : 0u;
    }
    for (uint32_t v = 1; v < rows; ++v) scan[v] += scan[v - 1];
    for (uint32_t v = 0; v < rows; ++v) cluster[v] = (uint32_t)(scan[root[v]] - 1u);
    return rows ? (uint32_t)scan[rows - 1u] : 0u;
}

// the sequential model: a union-find that knows nothing of the rule under test
struct Model {
    std::vector<uint32_t> parent, root, cluster;
    uint32_t count = 0;
    uint32_t find(uint32_t x) { while (parent[x] != x) x = parent[x] = parent[parent[x]]; return x; }
    Model(uint32_t rows, const std::vector<std::pair<uint32_t, uint32_t>> &edges) : parent(rows), root(rows), cluster(rows)
    {
        std::iota(parent.begin(), parent.end(), 0u);
        for (auto &e : edges) {
            const uint32_t a = find(e.first), b = find(e.second);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);
        }
        std::vector<uint32_t> id(rows);
        for (uint32_t v = 0; v < rows; ++v) {
            root[v] = find(v);
            if (root[v] == v) id[v] = count++;
        }
        for (uint32_t v = 0; v < rows; ++v) cluster[v] = id[root[v]];
    }
};

} // namespace

extern "C" {

// -> the number of (graph, order) pairs that differ from brute force or took more than `rows` steps in a link; *orders: how many ran
uint64_t ch_small(uint32_t max_rows, uint64_t *orders)
{
    uint64_t bad = 0, ran = 0;
    for (uint32_t n = 1; n <= max_rows; ++n) {
        std::vector<std::pair<uint32_t, uint32_t>> all;
        for (uint32_t a = 0; a < n; ++a)
            for (uint32_t b = a + 1; b < n; ++b) all.push_back({a, b});
        for (uint32_t mask = 0; mask < (1u << all.size()); ++mask) {
            std::vector<uint32_t> pick;
            for (uint32_t k = 0; k < all.size(); ++k)
                if (mask >> k & 1u) pick.push_back(k);
            // brute force: the smallest vertex each vertex reaches
            uint32_t reach[5];
            for (uint32_t v = 0; v < n; ++v) reach[v] = v;
            for (uint32_t round = 0; round < n; ++round)
                for (uint32_t k : pick) {
                    const uint32_t m = std::min(reach[all[k].first], reach[all[k].second]);
                    reach[all[k].first] = reach[all[k].second] = m;
                }
            do {
                std::atomic<uint32_t> parent[5];
                for (uint32_t v = 0; v < n; ++v) parent[v].store(v);
                AtomicParent par{parent};
                bool ok = true;
                uint32_t x = 0;
                for (uint32_t k : pick) { // (the orientation alternates along the order)
                    const uint32_t u = (x & 1u) ? all[k].second : all[k].first, v = (x & 1u) ? all[k].first : all[k].second;
                    ok &= components_link(par, u, v) <= n;
                    ++x;
                }
                uint32_t root[5], cluster[5], roots_below = 0;
                const uint32_t count = labels(par, n, root, cluster);
                for (uint32_t v = 0; v < n; ++v) {
                    ok &= root[v] == reach[v] && parent[v].load() <= v;
                    uint32_t below = 0;
                    for (uint32_t w = 0; w < reach[v]; ++w) below += reach[w] == w;
                    ok &= cluster[v] == below;
                    roots_below += reach[v] == v;
                }
                ok &= count == roots_below;
                bad += ok ? 0u : 1u;
                ++ran;
            } while (std::next_permutation(pick.begin(), pick.end()));
        }
    }
    if (orders) *orders = ran;
    return bad;
}

// -> 0, or a code of what differed; *max_steps: the most steps any link took
int ch_threads(uint64_t seed, uint32_t rows, uint32_t n_edges, uint32_t threads, uint32_t *max_steps)
{
    Rng rng{seed * 2654435761ull + 17u};
    std::vector<std::pair<uint32_t, uint32_t>> edges;
    for (uint32_t e = 0; e < n_edges; ++e) {
        const uint32_t a = rng.below(rows), b = rng.below(8u) == 0u ? a : rng.below(rows); // (one in eight a self-loop)
        edges.push_back({a, b});
        edges.push_back({b, a});
    }
    for (size_t i = edges.size(); i > 1; --i) std::swap(edges[i - 1], edges[rng.below((uint32_t)i)]);
    std::vector<std::atomic<uint32_t>> parent(rows + 2 * EDGE);
    for (auto &w : parent) w.store(GUARD);
    for (uint32_t v = 0; v < rows; ++v) parent[EDGE + v].store(v);
    AtomicParent par{parent.data() + EDGE};
    std::vector<uint32_t> steps(threads, 0u);
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            AtomicParent mine = par;
            for (size_t e = t; e < edges.size(); e += threads) steps[t] = std::max(steps[t], components_link(mine, edges[e].first, edges[e].second));
        });
    for (auto &th : pool) th.join();
    const uint32_t most = *std::max_element(steps.begin(), steps.end());
    if (max_steps) *max_steps = most;
    if (most > rows) return 1;
    std::vector<uint32_t> root(rows + 2 * EDGE, GUARD), cluster(rows + 2 * EDGE, GUARD);
    const uint32_t count = labels(par, rows, root.data() + EDGE, cluster.data() + EDGE);
    const Model model(rows, edges);
    if (count != model.count) return 2;
    for (uint32_t v = 0; v < rows; ++v) {
        if (root[EDGE + v] != model.root[v]) return 3;
        if (cluster[EDGE + v] != model.cluster[v]) return 4;
        if (parent[EDGE + v].load() > v) return 5;
    }
    for (size_t g = 0; g < EDGE; ++g)
        if (parent[g].load() != GUARD || parent[EDGE + rows + g].load() != GUARD || root[g] != GUARD || root[EDGE + rows + g] != GUARD ||
            cluster[g] != GUARD || cluster[EDGE + rows + g] != GUARD)
            return 6;
    return 0;
}

// -> the number of edges whose row the search gets wrong, over indptr arrays with empty rows at the front, in the middle, at the end
uint32_t ch_row_search()
{
    const std::vector<std::vector<uint32_t>> degrees = {
        {3}, {0, 0, 2}, {2, 0, 0}, {1, 0, 0, 0, 4, 0, 1}, {0, 0, 0, 5, 0, 0, 0}, {0, 1, 0, 1, 0, 1, 0}, {1, 1, 1, 1}, {0, 7}, {7, 0},
        {0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0}};
    uint32_t bad = 0;
    for (auto &deg : degrees) {
        std::vector<uint64_t> indptr(1, 0u);
        std::vector<uint32_t> row_of;
        for (uint32_t r = 0; r < deg.size(); ++r) {
            indptr.push_back(indptr.back() + deg[r]);
            row_of.insert(row_of.end(), deg[r], r);
        }
        for (uint64_t e = 0; e < row_of.size(); ++e) bad += components_edge_row(indptr.data(), (uint32_t)deg.size(), e) != row_of[e];
        // an edge number beyond indptr[rows] (a wrong indptr) still gives a row below `rows`
        bad += components_edge_row(indptr.data(), (uint32_t)deg.size(), row_of.size() + 5u) >= deg.size();
    }
    return bad;
}

uint32_t ch_link_grid(uint64_t nnz) { return components_link_grid(nnz); }

} // extern "C"

#ifdef COMPONENTS_HARNESS_MAIN
int main()
{
    uint64_t orders = 0;
    const uint64_t bad_small = ch_small(5u, &orders);
    uint32_t bad_threads = 0, most = 0;
    for (uint64_t seed = 1; seed <= 6; ++seed) {
        uint32_t steps = 0;
        bad_threads += ch_threads(seed, seed % 2 ? 2000u : 300u, seed % 3 ? 1000u : 4000u, 8u, &steps) != 0;
        most = std::max(most, steps);
    }
    const uint32_t bad_rows = ch_row_search();
    printf("%llu orders, %llu differ from brute force, %u threaded graphs differ, %u rows misplaced, at most %u steps in a link\n",
           (unsigned long long)orders, (unsigned long long)bad_small, bad_threads, bad_rows, most);
    return bad_small || bad_threads || bad_rows ? 1 : 0;
}
#endif
