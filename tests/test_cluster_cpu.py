"""components / cluster (the duplicate groups of a column as connected components) without a GPU: the exported symbols, every
argument error of the four entry points before any device, the link rule and the compress walk of strsim_components.h compiled by
g++ over std::atomic words (every edge order of every small graph, random graphs linked by 8 threads, the row search), the model of
tests/cluster_ref.py, and the Python surfaces with the context stubbed."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cluster_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "components_harness.cpp")
ERR_ARG = 2
COMPONENTS = ("strsim_components_device", "strsim_components_host")
CLUSTER = ("strsim_cluster_device", "strsim_cluster_host")
PLUGIN_NAMES = ("ratio", "token_sort_ratio", "levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")


@pytest.fixture(scope="module")
def L():
    import strsim_amd
    return strsim_amd.lib()  # (a library without strsim_components_device fails here: nothing is skipped)


def _build(out, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-pthread", "-I", CSRC, *flags, "-o", out, HARNESS])


@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="components_harness_")
    so = os.path.join(d.name, "libcomponents_harness.so")
    _build(so, "-fPIC", "-shared")
    lib = C.CDLL(so)
    lib.ch_small.restype = C.c_uint64
    lib.ch_small.argtypes = [C.c_uint32, C.POINTER(C.c_uint64)]
    lib.ch_threads.restype = C.c_int
    lib.ch_threads.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.ch_row_search.restype = C.c_uint32
    lib.ch_link_grid.restype = C.c_uint32
    lib.ch_link_grid.argtypes = [C.c_uint64]
    yield lib
    d.cleanup()


# ---- the rules -----------------------------------------------------------------------------------------------------------------

def test_components_every_edge_order_of_every_small_graph(H):
    orders = C.c_uint64(0)
    assert H.ch_small(5, C.byref(orders)) == 0
    # sum over n = 1 .. 5 and k of C(n (n - 1) / 2, k) * k! orders
    assert orders.value == 1 + 2 + 16 + 1957 + 9864101


@pytest.mark.parametrize("seed,rows,edges", [(1, 2000, 1000), (2, 300, 4000), (3, 5000, 2500), (4, 64, 64), (5, 1, 3), (6, 20000, 10000)])
def test_components_eight_threads_against_the_sequential_model(H, seed, rows, edges):
    steps = C.c_uint32(0)
    assert H.ch_threads(seed, rows, edges, 8, C.byref(steps)) == 0  # (1: a link took more than `rows` steps)
    assert steps.value <= rows


def test_components_row_search_over_empty_rows(H):
    assert H.ch_row_search() == 0


def test_components_link_grid_is_bounded(H):
    assert [H.ch_link_grid(n) for n in (1, 256, 257, 2 ** 21, 2 ** 21 + 1, 2 ** 40)] == [1, 1, 2, 8192, 8192, 8192]


def test_components_harness_stands_alone(tmp_path):
    # the same checks as a program of its own (the form that is run under the sanitizers)
    exe = str(tmp_path / "components_harness")
    _build(exe, "-DCOMPONENTS_HARNESS_MAIN")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 differ from brute force, 0 threaded graphs differ, 0 rows misplaced" in out.stdout


# ---- the model -------------------------------------------------------------------------------------------------------------------

def test_cluster_ref_components():
    # 0-3-5 chain given lower-only and upper-only, a self-loop, a duplicate, isolated rows
    indptr, index = [0, 1, 1, 2, 3, 3, 5, 5], [3, 2, 0, 3, 3]
    assert R.components(indptr, index) == ([0, 1, 2, 0, 4, 0, 6], [0, 1, 2, 0, 3, 0, 4], 5)
    assert R.components([0], []) == ([], [], 0)
    assert R.components([0, 0, 0], []) == ([0, 1], [0, 1], 2)
    assert R.components([0, 0, 1], [0]) == ([0, 0], [0, 0], 1)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_cluster_symbols_are_exported(L):
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    plug = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    for name in COMPONENTS:
        assert getattr(L, name) is not None
        assert "STRSIM_API int " + name + "(strsim_ctx_t *ctx, uint64_t rows, const uint64_t *indptr, const uint32_t *index, uint64_t nnz," in hdr
    for name in CLUSTER:
        assert getattr(L, name) is not None
        assert "STRSIM_API int " + name + "(strsim_ctx_t *ctx, int measure, const uint32_t *offsets, const uint8_t *values, uint64_t rows," in hdr
    for m in PLUGIN_NAMES:
        assert getattr(L, "_polars_plugin_cluster_" + m) is not None and getattr(L, "_polars_plugin_field_cluster_" + m) is not None
        assert "POLARS_PLUGIN_DECLARE(cluster_%s)" % m in plug


def test_cluster_leaves_the_abi_version_and_measure_supported_alone(L):
    assert L.strsim_abi_version() == 0x00010007
    for m in range(-1, 28):
        assert L.strsim_measure_supported(m, 3) == 0


def _components(L, name, rows=2, nnz=1, null=()):
    indptr = (C.c_uint64 * 3)(0, 1, 1)
    index = (C.c_uint32 * 1)(1)
    root = (C.c_uint32 * 2)(7, 7)
    cluster = (C.c_uint32 * 2)(7, 7)
    count = C.c_uint64(77)
    arg = lambda key, obj: None if key in null else C.addressof(obj)
    rc = getattr(L, name)(None, rows, arg("indptr", indptr), arg("index", index), nnz, arg("root", root), arg("cluster", cluster),
                          C.cast(arg("count", count), C.POINTER(C.c_uint64)))
    assert list(root) == [7, 7] and list(cluster) == [7, 7] and count.value == 77  # nothing is written on an argument error
    return rc


COMPONENTS_ERRORS = [
    ("too_many_rows", dict(rows=2 ** 32), "4294967296 rows (at most 2^32 - 1)"),
    ("null_indptr", dict(null=("indptr",)), "indptr is NULL"),
    ("null_index", dict(null=("index",)), "index is NULL with nnz=1"),
    ("null_root", dict(null=("root",)), "out_root is NULL"),
    ("null_count", dict(null=("count",)), "out_count is NULL"),
    ("rows_before_indptr", dict(rows=2 ** 33, null=("indptr", "count")), "8589934592 rows (at most 2^32 - 1)"),
    ("indptr_before_count", dict(null=("indptr", "count")), "indptr is NULL"),
]


@pytest.mark.parametrize("name", COMPONENTS)
@pytest.mark.parametrize("case,kw,msg", COMPONENTS_ERRORS)
def test_components_argument_errors_need_no_device(L, name, case, kw, msg):
    assert _components(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": " + msg


@pytest.mark.parametrize("name", COMPONENTS)
@pytest.mark.parametrize("kw", [dict(), dict(null=("cluster",)), dict(nnz=0, null=("index",)), dict(rows=0, nnz=0, null=("root", "cluster", "index")),
                                dict(rows=2 ** 32 - 1)])
def test_components_null_context_is_checked_last(L, name, kw):
    assert _components(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": ctx is NULL"


def _cluster(L, name, measure=2, rows=1, min_score=0.5, null=()):
    off = (C.c_uint32 * 2)(0, 1)
    val = (C.c_uint8 * 1)(97)
    root = (C.c_uint32 * 1)(7)
    cluster = (C.c_uint32 * 1)(7)
    count, nnz = C.c_uint64(77), C.c_uint64(78)
    arg = lambda key, obj: None if key in null else C.addressof(obj)
    rc = getattr(L, name)(None, measure, arg("off", off), arg("val", val), rows, min_score, arg("root", root), arg("cluster", cluster),
                          C.cast(arg("count", count), C.POINTER(C.c_uint64)), C.cast(arg("nnz", nnz), C.POINTER(C.c_uint64)))
    assert root[0] == 7 and cluster[0] == 7 and count.value == 77 and nnz.value == 78
    return rc


NOT_A_MEASURE = "measure %d is not a measure of cluster (the reference measures 0 .. 4, STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)"
CLUSTER_ERRORS = [
    ("measure5", dict(measure=5), NOT_A_MEASURE % 5),
    ("measure7", dict(measure=7), NOT_A_MEASURE % 7),
    ("measure16", dict(measure=16), NOT_A_MEASURE % 16),
    ("measure-1", dict(measure=-1), NOT_A_MEASURE % -1),
    ("nan", dict(min_score=float("nan")), "min_score is NaN"),
    ("measure_before_nan", dict(measure=9, min_score=float("nan")), NOT_A_MEASURE % 9),
    ("too_many_rows", dict(rows=2 ** 32 - 1), "4294967295 rows (at most 2^32 - 2)"),
    ("null_offsets", dict(null=("off",)), "NULL column buffer"),
    ("null_values", dict(null=("val",)), "NULL column buffer"),
    ("null_root", dict(null=("root",)), "out_root is NULL"),
    ("null_count", dict(null=("count",)), "out_count is NULL"),
    ("nan_before_rows", dict(min_score=float("nan"), rows=2 ** 40), "min_score is NaN"),
]


@pytest.mark.parametrize("name", CLUSTER)
@pytest.mark.parametrize("case,kw,msg", CLUSTER_ERRORS)
def test_cluster_argument_errors_need_no_device(L, name, case, kw, msg):
    assert _cluster(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": " + msg


@pytest.mark.parametrize("name", CLUSTER)
@pytest.mark.parametrize("measure", [0, 1, 2, 3, 4, 8, 14])
@pytest.mark.parametrize("kw", [dict(), dict(min_score=1.5), dict(min_score=-float("inf")), dict(null=("cluster",)), dict(null=("nnz",)),
                                dict(rows=0, null=("off", "val", "root", "cluster"))])
def test_cluster_null_context_is_checked_last(L, name, measure, kw):
    assert _cluster(L, name, measure=measure, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": ctx is NULL"


# ---- the Python surfaces ---------------------------------------------------------------------------------------------------------

def _decode(off, val):
    raw = bytes(val)
    return [raw[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


class _StubContext:
    """strsim_amd.cluster above Context.cluster: records the column it was sent and answers with fixed links"""
    def __init__(self, same):
        self.same = same  # strings that count as equal
        self.calls = []

    def cluster(self, measure, off, val, min_score):
        col = _decode(off, val)
        self.calls.append((measure, col, min_score))
        key = [self.same.get(s, s) for s in col]
        root = np.array([key.index(k) for k in key], dtype=np.uint32)
        firsts = sorted(set(root.tolist()))
        return root, np.array([firsts.index(r) for r in root], dtype=np.uint32), len(firsts)

    def default_process_host(self, off, val):
        raise AssertionError("no processor was asked for")


def test_cluster_python_surface():
    import strsim_amd
    from strsim_amd.context import Context
    for name in ("components", "cluster", "CLUSTER_MEASURES"):
        assert name in strsim_amd.__all__
    assert strsim_amd.CLUSTER_MEASURES == strsim_amd.MEASURES + ("ratio", "token_sort_ratio") == R.CLUSTER_MEASURES
    assert callable(Context.components) and callable(Context.cluster)
    for bad in ("osa", "wratio", "partial_ratio", 2, None):
        with pytest.raises(ValueError, match=r"no cluster by measure .*\(one of \('levenshtein', 'jaro', 'jaro_winkler', 'jaccard', 'sorensen_dice', "
                                             r"'ratio', 'token_sort_ratio'\)\)"):
            strsim_amd.cluster(bad, ["a"], 0.5)
    with pytest.raises(ValueError, match="min_score=None would put every row in one cluster"):
        strsim_amd.cluster("jaro", ["a"], None)
    with pytest.raises(ValueError, match="unknown processor 'lower'"):
        strsim_amd.cluster("jaro", ["a"], 0.5, processor="lower")


def test_cluster_null_mapping_with_a_stubbed_context():
    import strsim_amd
    col = [None, "anna", "", None, "ana", "bob", "", None, "anna"]
    stub = _StubContext({"ana": "anna"})
    root, label, count = strsim_amd.cluster("indel", col, 0.8, ctx=stub)
    # the nulls are not sent -- not even as empty strings, which would merge them with each other and with the real ones
    assert stub.calls == [("indel", ["anna", "", "ana", "bob", "", "anna"], 0.8)]
    assert root.dtype == label.dtype == np.int64
    assert root.tolist() == [-1, 1, 2, -1, 1, 5, 2, -1, 1]   # the caller's positions
    assert label.tolist() == [-1, 0, 1, -1, 0, 2, 1, -1, 0] and count == 3
    stub.calls.clear()
    assert strsim_amd.cluster("ratio", col, 0.8, ctx=stub)[0].tolist() == root.tolist() and stub.calls[0][0] == "indel"
    root, label, count = strsim_amd.cluster("jaro", [None, None], 0.8, ctx=stub)
    assert root.tolist() == [-1, -1] and label.tolist() == [-1, -1] and count == 0 and len(stub.calls) == 1
    root, label, count = strsim_amd.cluster("jaro", [], 0.8, ctx=stub)
    assert root.size == 0 and label.size == 0 and count == 0


def test_cluster_polars_wrapper_source():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert '__all__ += ["cluster"]' in src
    assert 'def cluster(expr: IntoExpr, measure: str = "jaro_winkler", min_score: float | None = None) -> pl.Expr:' in src
    body = src[src.index("def cluster("):]
    for word in ('df.with_columns(g=cluster("name", "jaro_winkler", 0.92)).group_by("g")', "a~b~c", "is_elementwise=False", '"cluster_" + measure',
                 "pl.lit(min_score, dtype=pl.Float64)", "UInt32"):
        assert word in body, word


@pytest.mark.parametrize("m", PLUGIN_NAMES)
def test_cluster_field_is_uint32_named_after_the_input(m):
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    assert arrow_host.field_plugin("cluster_" + m, ("name", "min_score")) == ("name", pa.uint32())
