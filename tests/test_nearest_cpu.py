"""Nearest match without a GPU: the exported symbols and version, argument errors before any device, the Python surface, the
plugin's field functions, the host builds of the two distance cores and of the sweep's window / skip / stop rules
(strsim_nearest.h), and the NumPy reference top-k of the GPU tests against a brute-force sort."""
import ctypes as C
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import distance_ref as D
import nearest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "nearest_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
ERR_ARG = 2
U = R.UNBOUNDED


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    vp, u64 = C.c_void_p, C.c_uint64
    for name in ("strsim_nearest_device", "strsim_nearest_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp]
    L.strsim_abi_version.restype = C.c_uint32
    L.strsim_last_error_message.restype = C.c_char_p
    return L


@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="nearest_harness_")
    so = os.path.join(d.name, "libnearest_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.nearest_core.restype = C.c_uint32
    L.nearest_core.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, C.c_int]
    L.nearest_wave.restype = C.c_uint64
    L.nearest_wave.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp]
    L.nearest_plan.restype = None
    L.nearest_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.nearest_needs_h.restype = C.c_int
    L.nearest_needs_h.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32]
    yield L
    d.cleanup()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

def test_nearest_keeps_abi_version_1_7(L):
    assert L.strsim_abi_version() == 0x00010007
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    assert re.search(r"#define STRSIM_ABI_VERSION 0x00010007u", hdr)
    assert re.search(r"#define STRSIM_NEAREST_MAX_K 16u", hdr)


def test_nearest_symbols_are_exported(L):
    for name in ("strsim_nearest_device", "strsim_nearest_host", "_polars_plugin_nearest_levenshtein", "_polars_plugin_nearest_osa",
                 "_polars_plugin_field_nearest_levenshtein", "_polars_plugin_field_nearest_osa"):
        assert getattr(L, name) is not None
    hdr = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    assert "POLARS_PLUGIN_DECLARE(nearest_levenshtein)" in hdr and "POLARS_PLUGIN_DECLARE(nearest_osa)" in hdr


def _nearest_call(L, name, k=1, q_rows=1, c_rows=1, measure=0, null_q=False, null_out=False, null_c=False, null_cv=False):
    qo = (C.c_uint32 * 2)(0, 1)
    qv = (C.c_uint8 * 1)(97)
    idx = (C.c_uint32 * 32)()
    dist = (C.c_uint32 * 32)()
    f = getattr(L, name)
    return f(None, measure, None if null_q else C.addressof(qo), C.addressof(qv), q_rows, None if null_c else C.addressof(qo),
             None if null_cv else C.addressof(qv), c_rows, k, U, None if null_out else C.addressof(idx),
             None if null_out else C.addressof(dist))


@pytest.mark.parametrize("name", ["strsim_nearest_device", "strsim_nearest_host"])
@pytest.mark.parametrize("case,kw,msg", [
    ("k0", dict(k=0), "k=0"),
    ("k17", dict(k=17), "k=17"),
    ("measure1", dict(measure=1), "measure 1"),
    ("measure5", dict(measure=5), "measure 5"),
    ("measure7", dict(measure=7), "measure 7"),
    ("null_queries", dict(null_q=True), "NULL"),
    ("null_outputs", dict(null_out=True), "NULL"),
    ("null_candidates", dict(null_c=True), "NULL"),
    ("null_candidate_values", dict(null_cv=True), "NULL"),
    ("too_many_candidates", dict(c_rows=2 ** 32 - 1), "candidates"),
    ("too_many_queries", dict(q_rows=2 ** 32), "queries"),
])
def test_nearest_argument_errors_need_no_device(L, name, case, kw, msg):
    # the arguments are checked before the context: STRSIM_ERR_ARG, with the reason in the message, on a box without a GPU
    assert _nearest_call(L, name, **kw) == ERR_ARG
    assert msg in L.strsim_last_error_message().decode()


@pytest.mark.parametrize("name", ["strsim_nearest_device", "strsim_nearest_host"])
@pytest.mark.parametrize("measure", [0, 6])
def test_nearest_null_context_is_an_argument_error(L, name, measure):
    assert _nearest_call(L, name, k=16, measure=measure) == ERR_ARG
    assert "ctx is NULL" in L.strsim_last_error_message().decode()


# ---- Python surface and plugin fields ---------------------------------------------------------------------------------------

def test_nearest_python_surface():
    import strsim_amd
    from strsim_amd.context import Context
    assert "nearest" in strsim_amd.__all__ and callable(strsim_amd.nearest)
    assert callable(Context.nearest)
    for bad in ("jaro", "jaccard", "best_match", 1):
        with pytest.raises(ValueError, match="no distance"):
            strsim_amd.nearest(bad, ["a"], ["b"])
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert re.search(r'__all__ = \[[^\]]*"nearest"', src)
    assert "def nearest(expr: IntoExpr, candidates: IntoExpr, measure: str = \"levenshtein\", max_distance" in src


@pytest.mark.parametrize("fn", ["nearest_levenshtein", "nearest_osa"])
def test_nearest_field_is_index_distance_struct_named_after_first_input(fn):
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    want = pa.struct([pa.field("index", pa.uint32()), pa.field("distance", pa.uint32())])
    assert arrow_host.field_plugin(fn, ("queries", "cands")) == ("queries", want)
    assert arrow_host.field_plugin(fn, ("q", "c", "max_distance")) == ("q", want)


def test_best_match_field_is_unchanged():
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    want = pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])
    assert arrow_host.field_plugin("best_match_levenshtein", ("queries", "cands")) == ("queries", want)


# ---- host builds of the shared kernel code ----------------------------------------------------------------------------------

def _rand_ascii(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


@pytest.mark.parametrize("measure", ["levenshtein", "osa"])
def test_nearest_core_every_length_pair(H, measure):
    # the uniform-text core of k_nearest_lane against distance_ref, query and candidate lengths 0..32, seven planes on mixed-case
    # ASCII (bit 5 and 6 vary) and five planes on lowercase (they do not)
    rng = random.Random(13 + len(measure))
    tr = 1 if measure == "osa" else 0
    A, B, got7, got5, A5, B5 = [], [], [], [], [], []
    for lq in range(33):
        for lc in range(33):
            a, b = _rand_ascii(rng, lq, "abAB1 ~"), _rand_ascii(rng, lc, "abAB1 ~")
            if lc and lq and rng.random() < 0.3:
                b = (a[:lc] + b)[:lc]  # near copies: small distances
            A.append(a); B.append(b)
            got7.append(H.nearest_core(a.encode(), lq, b.encode(), lc, 7, tr))
            a5, b5 = _rand_ascii(rng, lq, "abcz"), _rand_ascii(rng, lc, "abcz")
            A5.append(a5); B5.append(b5)
            got5.append(H.nearest_core(a5.encode(), lq, b5.encode(), lc, 5, tr))
    assert np.array_equal(np.array(got7, dtype=np.uint32), D.batch_numpy(measure, A, B))
    assert np.array_equal(np.array(got5, dtype=np.uint32), D.batch_numpy(measure, A5, B5))


def test_nearest_core_transposition_cases(H):
    for a, b, lev, osa in (("ab", "ba", 2, 1), ("ca", "abc", 3, 3), ("abcdef", "badcfe", 4, 3), ("", "xyz", 3, 3), ("xyz", "", 3, 3)):
        assert H.nearest_core(a.encode(), len(a), b.encode(), len(b), 7, 0) == lev
        assert H.nearest_core(a.encode(), len(a), b.encode(), len(b), 7, 1) == osa


def _plan(H, lmin, lmax, kmax):
    out = (C.c_uint32 * (3 + 4 * 40))()
    H.nearest_plan(lmin, lmax, kmax, C.addressof(out))
    lo, hi, steps = out[0], out[1], out[2]
    order = []
    for g in range(steps):
        f, l, s, any_ = out[3 + 4 * g: 7 + 4 * g]
        if any_:
            order.append(list(range(f, l + 1, s)))
        else:
            order.append([])
    return lo, hi, order


@pytest.mark.parametrize("kmax", [0, 1, 2, 3, 5, 16, 31, 32, U])
def test_nearest_window_and_order_cover_exactly_the_window(H, kmax):
    # every (lmin, lmax): the window is [lmin - kmax, lmax + kmax] within 0..32, the nearest-first order visits each of its
    # lengths exactly once, and every length of step g is exactly g away from [lmin, lmax]
    for lmin in range(33):
        for lmax in range(lmin, 33):
            lo, hi, order = _plan(H, lmin, lmax, kmax)
            k = 10 ** 9 if kmax == U else kmax
            assert (lo, hi) == (max(0, lmin - k), min(32, lmax + k))
            flat = [L for step in order for L in step]
            assert sorted(flat) == list(range(lo, hi + 1))
            for g, step in enumerate(order):
                for L in step:
                    gap = 0 if lmin <= L <= lmax else (lmin - L if L < lmin else L - lmax)
                    assert gap == g


def test_nearest_needs_is_strict_about_the_bound(H):
    # |lq - lc| <= b is needed; b = min(kmax, K-th distance); an empty K-th slot leaves b = kmax
    EMPTY = 2 ** 64 - 1
    for lq in range(33):
        for lc in range(33):
            gap = abs(lq - lc)
            for dk in range(0, 6):
                for kmax in (0, 2, 4, U):
                    key = (dk << 32) | 7
                    b = min(dk, kmax)
                    assert H.nearest_needs_h(lq, lc, key, kmax) == int(gap <= b)
                assert H.nearest_needs_h(lq, lc, EMPTY, dk) == int(gap <= dk)
            assert H.nearest_needs_h(lq, lc, EMPTY, U) == 1


def _wave(H, qlen, clen, dist, K, kmax):
    nq, nc = len(qlen), len(clen)
    ql = np.ascontiguousarray(qlen, dtype=np.uint32)
    cl = np.ascontiguousarray(clen, dtype=np.uint32)
    dm = np.ascontiguousarray(dist, dtype=np.uint32)
    oi = np.zeros((nq, K), dtype=np.uint32)
    od = np.zeros((nq, K), dtype=np.uint32)
    visited = H.nearest_wave(ql.ctypes.data, nq, cl.ctypes.data, nc, dm.ctypes.data, K, kmax, oi.ctypes.data, od.ctypes.data)
    idx = np.where(oi == 0xFFFFFFFF, -1, oi.astype(np.int64))
    d = np.where(oi == 0xFFFFFFFF, -1, od.astype(np.int64))
    return idx, d, visited


@pytest.mark.parametrize("seed", range(12))
def test_nearest_sweep_rules_match_brute_force(H, seed):
    # one wave's sweep with the window, skip and stop rules against a full sort, on distances d >= |lq - lc| with many ties
    rng = np.random.default_rng(seed)
    lbase = int(rng.integers(0, 33))
    nq = int(rng.integers(1, 65))
    qlen = np.clip(lbase + rng.integers(0, 2, size=nq), 0, 32)
    nc = int(rng.integers(0, 300))
    clen = rng.integers(0, 33, size=nc)
    gap = np.abs(qlen[:, None] - clen[None, :])
    dist = gap + rng.integers(0, 3, size=(nq, nc)) * rng.integers(0, 2, size=(nq, nc))
    for K in (1, 4, 16):
        for kmax in (0, 1, 2, 5, U):
            idx, d, visited = _wave(H, qlen, clen, dist, K, kmax)
            ri, rd = R.brute_topk(dist, K, kmax)
            assert np.array_equal(idx, ri), (K, kmax)
            assert np.array_equal(d, rd), (K, kmax)
            assert visited <= nc


def test_nearest_sweep_admits_a_tie_of_the_kth_distance_with_a_lower_index(H):
    # query length 4, K = 4: length 4 fills three slots, length 2 (two away) brings the fourth; then the list is full with the
    # bound b = 2, and length 7 (three away) is never visited
    clen = np.array([2, 4, 4, 4, 7], dtype=np.uint32)
    qlen = np.array([4], dtype=np.uint32)
    dist = np.array([[2, 2, 1, 2, 3]], dtype=np.uint32)
    idx, d, visited = _wave(H, qlen, clen, dist, 4, U)
    assert idx.tolist() == [[2, 0, 1, 3]] and d.tolist() == [[1, 2, 2, 2]]
    # K = 1 with a tie at the bound: the length-2 candidate (index 0, d = 2) ties (2, index 1) and must win
    dist = np.array([[2, 2, 3, 3, 3]], dtype=np.uint32)
    idx, d, _ = _wave(H, qlen, clen, dist, 1, U)
    assert idx.tolist() == [[0]] and d.tolist() == [[2]]
    # and the dynamic bound prunes: a d = 0 match at the query's own length ends the sweep before any other length
    dist = np.array([[2, 0, 1, 1, 3]], dtype=np.uint32)
    idx, d, visited = _wave(H, qlen, clen, dist, 1, U)
    assert idx.tolist() == [[1]] and d.tolist() == [[0]] and visited == 3


# ---- the NumPy reference --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_nearest_reference_topk_matches_a_brute_force_sort(seed):
    rng = np.random.default_rng(seed)
    n, m = 7, int(rng.integers(0, 40))
    dist = rng.integers(0, 5, size=(n, m))  # many ties
    for k in (1, 3, 16):
        for md in (None, 0, 1, 2, 4, U):
            a = R.topk(dist, k, md)
            b = R.brute_topk(dist, k, md)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_nearest_reference_topk_order_and_cutoff():
    d = np.array([[3, 1, 3, 1, 0, 5]])
    idx, val = R.topk(d, 4)
    assert idx.tolist() == [[4, 1, 3, 0]] and val.tolist() == [[0, 1, 1, 3]]
    idx, val = R.topk(d, 7, 1)
    assert idx.tolist() == [[4, 1, 3, -1, -1, -1, -1]] and val.tolist() == [[0, 1, 1, -1, -1, -1, -1]]
    idx, val = R.topk(d, 2, 0)
    assert idx.tolist() == [[4, -1]]


def test_nearest_reference_distance_matrix():
    q, c = ["abc", "", "ab"], ["abcdefgh", "xyz", "", "ba"]
    M = R.distance_matrix("levenshtein", q, c)
    assert M.tolist() == [[5, 3, 3, 2], [8, 3, 0, 2], [6, 3, 2, 2]]
    assert R.distance_matrix("osa", q, c)[2, 3] == 1
