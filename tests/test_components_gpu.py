"""strsim_components_device / _host on the GPU, exact against the union-find of tests/cluster_ref.py: roots, dense ids and count
through both entry points, for graphs that force long chains across workgroups (paths), contention on one root (a star whose centre
is the highest index), many hooks per vertex (cliques, duplicates, self-loops), the giant-component threshold of a random graph and
many small components."""
import ctypes as C
import random

import numpy as np
import pytest

import cluster_ref as R
import strsim_amd as S

pytestmark = pytest.mark.gpu
ERR_ARG = 2
GUARD = 0x5EA1F00D


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def csr(rows, edges):
    """(u, v) pairs as given (directed storage) -> (indptr uint64 [rows + 1], index uint32 [nnz]); the order inside a row is kept"""
    per = [[] for _ in range(rows)]
    for u, v in edges:
        per[u].append(v)
    indptr = np.zeros(rows + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum([len(p) for p in per], dtype=np.uint64)
    return indptr, np.array([v for p in per for v in p], dtype=np.uint32)


def _device(torch, indptr, index):
    dev = torch.device("cuda", 0)
    ip = torch.from_numpy(indptr.view(np.int64)).to(dev)
    ix = torch.from_numpy(np.ascontiguousarray(index).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    return ip, ix


def check_both(ctx, rows, edges, what=""):
    """both entry points against the model; -> the model's (root, cluster, count)"""
    torch = pytest.importorskip("torch")
    indptr, index = csr(rows, edges)
    exp = R.components(indptr, index, rows)
    root, cluster, count = ctx.components(indptr, index, rows)
    assert root.dtype == np.uint32 and cluster.dtype == np.uint32
    assert count == exp[2], "%s host: count" % what
    assert root.tolist() == exp[0], "%s host: roots" % what
    assert cluster.tolist() == exp[1], "%s host: dense ids" % what
    root, cluster, count = ctx.components(*_device(torch, indptr, index), rows)
    assert root.is_cuda and cluster.is_cuda and root.dtype == torch.int32 and cluster.dtype == torch.int32
    assert count == exp[2], "%s device: count" % what
    assert root.cpu().tolist() == exp[0], "%s device: roots" % what
    assert cluster.cpu().tolist() == exp[1], "%s device: dense ids" % what
    return exp


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 257])
def test_components_gpu_no_edges_is_the_identity(ctx, rows):
    exp = check_both(ctx, rows, [])
    assert exp == (list(range(rows)), list(range(rows)), rows)


def test_components_gpu_zero_rows(ctx):
    root, cluster, count = ctx.components(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    assert root.size == 0 and cluster.size == 0 and count == 0


PATH_ROWS = 4097


@pytest.mark.parametrize("form", ["in_order", "shuffled_and_flipped", "lower_only"])
def test_components_gpu_path_across_workgroups(ctx, form):
    edges = [(v, v + 1) for v in range(PATH_ROWS - 1)]
    if form == "shuffled_and_flipped":
        rng = random.Random(5)
        rng.shuffle(edges)
        edges = [(b, a) if rng.random() < 0.5 else (a, b) for a, b in edges]
    elif form == "lower_only":
        edges = [(b, a) for a, b in edges]
    exp = check_both(ctx, PATH_ROWS, edges, form)
    assert exp[2] == 1 and set(exp[0]) == {0}


@pytest.mark.parametrize("two_sided", [False, True])
def test_components_gpu_star_with_the_centre_at_the_highest_index(ctx, two_sided):
    # every hook contends for the centre's root: the compare-and-swap fails and the link goes on from the new parents
    leaves = 5000
    edges = [(v, leaves) for v in range(leaves)]  # upper-only: the leaf rows hold the centre
    if two_sided:
        edges += [(leaves, v) for v in range(leaves)]
    exp = check_both(ctx, leaves + 1, edges)
    assert exp[2] == 1
    # isolated rows around the star keep their own ids
    exp = check_both(ctx, leaves + 4, [(v + 2, leaves + 2) for v in range(leaves)])
    assert exp[2] == 4 and exp[0][:3] == [0, 1, 2] and exp[1][-1] == 3


@pytest.mark.parametrize("noisy", [False, True])
def test_components_gpu_clique(ctx, noisy):
    n = 300
    edges = [(a, b) for a in range(n) for b in range(a + 1, n)]
    if noisy:
        edges = edges + edges + [(v, v) for v in range(n)]
    exp = check_both(ctx, n, edges)
    assert exp[2] == 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_components_gpu_random_graph_at_the_giant_component_threshold(ctx, seed):
    rows, m = 20000, 10000
    rng = random.Random(seed)
    edges = [(rng.randrange(rows), rng.randrange(rows)) for _ in range(m)]
    exp = check_both(ctx, rows, edges)
    sizes = np.bincount(np.array(exp[0]))
    assert sizes.max() > 20 and exp[2] >= rows - m  # a large component next to thousands of small ones (every edge merges at most two)


def test_components_gpu_disjoint_triangles_are_numbered_by_first_member(ctx):
    t = 1000
    order = list(range(3 * t))
    random.Random(9).shuffle(order)  # triangle k is rows order[3k .. 3k + 3)
    edges = []
    for k in range(t):
        a, b, c = order[3 * k:3 * k + 3]
        edges += [(a, b), (c, b), (a, c)]
    exp = check_both(ctx, 3 * t, edges)
    assert exp[2] == t
    firsts = sorted(min(order[3 * k:3 * k + 3]) for k in range(t))
    assert [exp[1][f] for f in firsts] == list(range(t))


def test_components_gpu_launch_count_does_not_depend_on_the_graph(ctx):
    torch = pytest.importorskip("torch")
    L = S.lib()
    ops = lambda: L.strsim_ctx_enqueued_ops(ctx._h)
    rows = 300
    path = _device(torch, *csr(rows, [(v, v + 1) for v in range(rows - 1)]))
    clique = _device(torch, *csr(rows, [(a, b) for a in range(rows) for b in range(a + 1, rows)]))
    none = _device(torch, *csr(rows, []))
    ctx.synchronize()
    n0 = ops()
    ctx.components(*path, rows)
    n1 = ops()
    ctx.components(*clique, rows)
    n2 = ops()
    ctx.components(*none, rows)
    n3 = ops()
    # init, link, compress, three scan kernels, rank and the 16-byte copy; without edges one launch
    assert (n1 - n0, n2 - n1, n3 - n2) == (8, 8, 1)


def _guarded(n):
    a = np.full(n + 16, GUARD, dtype=np.uint32)
    return a, a[8:8 + n]


def test_components_gpu_index_out_of_range(ctx):
    torch = pytest.importorskip("torch")
    L = S.lib()
    rows = 100
    indptr, index = csr(rows, [(v, v + 1) for v in range(rows - 1)] + [(rows - 1, rows), (3, 2 ** 32 - 1)])  # an index == rows, and a huge one
    exp = R.components(*csr(rows, [(v, v + 1) for v in range(rows - 1)]), rows)
    count = C.c_uint64(0)
    # host entry point
    root_all, root = _guarded(rows)
    cl_all, cl = _guarded(rows)
    rc = L.strsim_components_host(ctx._h, rows, indptr.ctypes.data, index.ctypes.data, index.size, root.ctypes.data, cl.ctypes.data, C.byref(count))
    assert rc == ERR_ARG
    msg = L.strsim_last_error_message().decode()
    assert msg.startswith("strsim_components_host: index out of range (2 of 101 edges"), msg
    assert (root_all[:8] == GUARD).all() and (root_all[-8:] == GUARD).all() and (cl_all[:8] == GUARD).all() and (cl_all[-8:] == GUARD).all()
    # device entry point: the bad edges are skipped, the labels of the others are written, the guards stand
    dev = torch.device("cuda", 0)
    ip, ix = _device(torch, indptr, index)
    d_root = torch.from_numpy(np.full(rows + 16, GUARD, dtype=np.uint32).view(np.int32)).to(dev)
    d_cl = d_root.clone()
    rc = L.strsim_components_device(ctx._h, rows, ip.data_ptr(), ix.data_ptr(), index.size, d_root.data_ptr() + 32, d_cl.data_ptr() + 32, C.byref(count))
    assert rc == ERR_ARG
    msg = L.strsim_last_error_message().decode()
    assert msg.startswith("strsim_components_device: index out of range (2 of 101 edges"), msg
    ctx.synchronize()
    got_root, got_cl = d_root.cpu().numpy().view(np.uint32), d_cl.cpu().numpy().view(np.uint32)
    for a in (got_root, got_cl):
        assert (a[:8] == GUARD).all() and (a[-8:] == GUARD).all()
    assert got_root[8:-8].tolist() == exp[0] and got_cl[8:-8].tolist() == exp[1]
    with pytest.raises(S.StrsimError, match="index out of range"):
        ctx.components(indptr, index, rows)


def test_components_gpu_without_out_cluster(ctx):
    torch = pytest.importorskip("torch")
    L = S.lib()
    rows = 500
    rng = random.Random(11)
    indptr, index = csr(rows, [(rng.randrange(rows), rng.randrange(rows)) for _ in range(300)])
    exp = R.components(indptr, index, rows)
    count = C.c_uint64(0)
    root_all, root = _guarded(rows)
    assert L.strsim_components_host(ctx._h, rows, indptr.ctypes.data, index.ctypes.data, index.size, root.ctypes.data, None, C.byref(count)) == 0
    assert root.tolist() == exp[0] and count.value == exp[2] and (root_all[:8] == GUARD).all() and (root_all[-8:] == GUARD).all()
    ip, ix = _device(torch, indptr, index)
    d_root = torch.empty(rows, dtype=torch.int32, device=ip.device)
    count = C.c_uint64(0)
    assert L.strsim_components_device(ctx._h, rows, ip.data_ptr(), ix.data_ptr(), index.size, d_root.data_ptr(), None, C.byref(count)) == 0
    assert d_root.cpu().tolist() == exp[0] and count.value == exp[2]
    # and without edges
    assert L.strsim_components_device(ctx._h, rows, ip.data_ptr(), None, 0, d_root.data_ptr(), None, C.byref(count)) == 0
    ctx.synchronize()
    assert d_root.cpu().tolist() == list(range(rows)) and count.value == rows


def test_components_gpu_python_surface(ctx):
    # the CSR of an upper self-join as it is
    indptr, index, _ = S.join("ratio", ["anna", "bob", "anne", "bobby", "ann", "zed"], ["anna", "bob", "anne", "bobby", "ann", "zed"], 0.7, upper=True, ctx=ctx)
    root, cluster, count = S.components(indptr, index, ctx=ctx)
    assert root.dtype == cluster.dtype == np.int64
    assert root.tolist() == [0, 1, 0, 1, 0, 5] and cluster.tolist() == [0, 1, 0, 1, 0, 2] and count == 3
