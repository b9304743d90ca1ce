"""cdist (the full score matrix) without a GPU: the exported symbols and version, argument errors before any device, the Python
surface with the context stubbed, the plugin's field functions, and the host build of the rules k_cdist_lane shares with the host
(strsim_cdist.h): the store schedule of a wave's tile replayed over an array with guard words, the 64-bit index, the split rule and
the Indel score table."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import cdist_ref as R
import indel_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "cdist_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
ERR_ARG = 2
INF = float("inf")
NAMES = ("strsim_cdist_device", "strsim_cdist_host")
PLUGIN = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice", "ratio", "token_sort_ratio")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    vp, u64 = C.c_void_p, C.c_uint64
    for name in NAMES:
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, C.c_double, vp, u64]
    L.strsim_abi_version.restype = C.c_uint32
    L.strsim_last_error_message.restype = C.c_char_p
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_measure_supported.argtypes = [C.c_int, C.c_int]
    return L


def _build(out, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, *flags, "-o", out, HARNESS])


@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="cdist_harness_")
    so = os.path.join(d.name, "libcdist_harness.so")
    _build(so, "-fPIC", "-shared")
    L = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    L.cdist_replay.restype = C.c_int
    L.cdist_replay.argtypes = [u32, u32, u32, u32, u32]
    L.cdist_replay_all.restype = u32
    L.cdist_index_h.restype = u64
    L.cdist_index_h.argtypes = [u64, u64, u64]
    L.cdist_item_h.restype = u32
    L.cdist_item_h.argtypes = [u32, u64, u32, u32, u64, u32, u32]
    L.cdist_splits_h.restype = u32
    L.cdist_splits_h.argtypes = [u64, u64, C.c_int]
    L.cdist_tj.restype = u32
    L.cdist_block.restype = u32
    L.cdist_table_score.restype = C.c_double
    L.cdist_table_score.argtypes = [u32, u32]
    L.cdist_epilogue.restype = C.c_double
    L.cdist_epilogue.argtypes = [u32, u32]
    L.cdist_cut_h.restype = C.c_double
    L.cdist_cut_h.argtypes = [C.c_double, C.c_double]
    yield L
    d.cleanup()


# ---- the store schedule -------------------------------------------------------------------------------------------------------

def test_cdist_tile_schedule_writes_every_element_once_and_no_guard(H):
    # q in 0..130, c in 0..40, ld - c in {0, 1, 3}, the base 16-byte aligned and 8 bytes past it, 1..4 splits: every (i, j) is
    # written exactly once with its own value, every 16-byte store is aligned, no guard word is touched
    assert H.cdist_replay_all() == 0


@pytest.mark.parametrize("q,c,pad,mis,splits", [(1, 1, 0, 0, 1), (64, 16, 0, 1, 1), (65, 17, 1, 1, 2), (130, 40, 3, 0, 4), (130, 40, 3, 1, 3),
                                                (257, 35, 1, 1, 4), (63, 33, 0, 1, 2), (300, 100, 3, 1, 4)])
def test_cdist_tile_schedule_cases(H, q, c, pad, mis, splits):
    assert H.cdist_replay(q, c, pad, mis, splits) == 0


def test_cdist_items_pair_up_on_16_byte_boundaries(H):
    # a row whose first double is 16-byte aligned is TJ / 2 pairs; one that is not is a single, TJ / 2 - 1 pairs and a single
    tj = H.cdist_tj()
    assert tj in (8, 16)
    slots = tj // 2 + 1
    for base8, want in ((0, [2] * (tj // 2) + [0]), (1, [1] + [2] * (tj // 2 - 1) + [1])):
        items = [H.cdist_item_h(t, base8, 0, 64, tj, 0, tj) for t in range(slots)]
        assert [x >> 16 for x in items] == want and all((x & 0xFF) == 0 for x in items)
        cols = [(x >> 8) & 0xFF for x, n in zip(items, want) if n]
        assert cols == [sum(want[:k]) for k in range(slots) if want[k]]
    # an odd leading dimension alternates the phase row by row; rows at and above `rows` store nothing
    assert [H.cdist_item_h(r * slots, 0, 0, 64, tj + 1, 0, tj) >> 16 for r in range(4)] == [2, 1, 2, 1]
    assert H.cdist_item_h(5 * slots, 0, 0, 5, tj, 0, tj) >> 16 == 0 and H.cdist_item_h(4 * slots, 0, 0, 5, tj, 0, tj) >> 16 == 2
    # a tile cut short at n columns
    assert [H.cdist_item_h(t, 0, 0, 64, tj, 0, 3) >> 16 for t in range(slots)] == [2, 1] + [0] * (slots - 2)


def test_cdist_index_is_exact_in_64_bits(H):
    big = 2 ** 32 - 2
    assert H.cdist_index_h(big, big, big - 1) == big * big + big - 1
    assert H.cdist_index_h(2 ** 32 - 2, 2 ** 32 - 2, 0) == (2 ** 32 - 2) ** 2
    assert H.cdist_index_h(3, 7, 2) == 23
    # the phase of a row far out: the item's parity follows the exact index
    tj = H.cdist_tj()
    for i0 in (2 ** 32 - 66, 2 ** 32 - 65):
        for ld in (2 ** 32 - 2, 2 ** 32 - 3):
            h = (1 + i0 * ld + 5) & 1
            assert H.cdist_item_h(0, 1, i0, 64, ld, 5, tj) >> 16 == (1 if h else 2)


def test_cdist_splits_fill_the_device_and_keep_four_tiles(H):
    # about four workgroups per CU over the query workgroups, never less than four tiles of candidates per split
    tj, block = H.cdist_tj(), H.cdist_block()
    assert block in (256, 512, 1024)

    def want(nq, nc, cu=256):
        qblocks = -(-nq // block)
        return max(1, min(-(-4 * cu // qblocks), -(-nc // (4 * tj)), 65535))
    for nq, nc in ((5, 3000), (300, 700), (20000, 10000), (10 ** 6, 10 ** 6), (1, 1), (1, 2 ** 32 - 2), (2 ** 32 - 1, 5)):
        assert H.cdist_splits_h(nq, nc, 256) == want(nq, nc), (nq, nc)
    assert H.cdist_splits_h(5, 3000, 256) == -(-3000 // (4 * tj))  # few queries: as many splits as four tiles allow
    assert H.cdist_splits_h(10 ** 6, 10 ** 6, 256) == 1             # enough query workgroups: no split
    assert H.cdist_splits_h(1, 2 ** 32 - 2, 256) == 1024 and H.cdist_splits_h(7, 10 ** 9, 0) == 1024 and H.cdist_splits_h(7, 10 ** 9, 64) == 256


def test_cdist_harness_stands_alone(tmp_path):
    # the same sweep as a program of its own (the form that is run under the sanitizers)
    exe = str(tmp_path / "cdist_harness")
    _build(exe, "-DCDIST_HARNESS_MAIN")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 shapes failed, 0 table entries differ, 64-bit index exact" in out.stdout


# ---- the Indel score table and the cutoff rule -----------------------------------------------------------------------------------

def test_cdist_indel_table_is_epilogue_indel_at_every_pair(H):
    n = 0
    for s in range(65):
        for d in range(s + 1):
            v = H.cdist_table_score(d, s)
            assert v == H.cdist_epilogue(d, s) == indel_ref.normalise(d, s, 0)
            n += 1
    assert n == 2145
    assert H.cdist_table_score(0, 0) == 1.0 and H.cdist_table_score(2, 4) == 0.5 and H.cdist_table_score(5, 5) == 0.0


def test_cdist_cutoff_rule(H):
    import math
    assert H.cdist_cut_h(0.5, 0.5) == 0.5 and H.cdist_cut_h(0.5, math.nextafter(0.5, INF)) == 0.0
    assert H.cdist_cut_h(0.5, math.nextafter(0.5, -INF)) == 0.5
    assert H.cdist_cut_h(0.0, -INF) == 0.0 and H.cdist_cut_h(0.25, 0.0) == 0.25 and H.cdist_cut_h(1.0, 1.0) == 1.0
    assert H.cdist_cut_h(1.0, 1.5) == 0.0
    M = np.array([[0.5, 0.25], [1.0, 0.0]])
    assert R.apply_cutoff(M, 0.5).tolist() == [[0.5, 0.0], [1.0, 0.0]] and R.apply_cutoff(M, None) is M


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_cdist_keeps_abi_version_1_7(L):
    assert L.strsim_abi_version() == 0x00010007
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    assert re.search(r"#define STRSIM_ABI_VERSION 0x00010007u", hdr)
    for name in NAMES:
        assert re.search(r"STRSIM_API int " + name + r"\(strsim_ctx_t \*ctx, int measure,", hdr)


def test_cdist_symbols_are_exported(L):
    hdr = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    for name in NAMES:
        assert getattr(L, name) is not None
    for m in PLUGIN:
        assert getattr(L, "_polars_plugin_cdist_" + m) is not None and getattr(L, "_polars_plugin_field_cdist_" + m) is not None
        assert "POLARS_PLUGIN_DECLARE(cdist_%s)" % m in hdr


def test_cdist_leaves_measure_supported_alone(L):
    for m in (8, 10, 14, 16):
        assert L.strsim_measure_supported(m, 1) == 0 and L.strsim_measure_supported(m, 0) == 1
    for m in range(5):
        assert L.strsim_measure_supported(m, 1) == 1
    for m in range(-1, 18):
        assert L.strsim_measure_supported(m, 3) == 0


def _call(L, name, measure=8, q_rows=1, c_rows=1, cutoff=-INF, ld=None, null_q=False, null_qv=False, null_c=False, null_cv=False, null_out=False):
    qo = (C.c_uint32 * 2)(0, 1)
    qv = (C.c_uint8 * 1)(97)
    out = (C.c_double * 8)()
    f = getattr(L, name)
    return f(None, measure, None if null_q else C.addressof(qo), None if null_qv else C.addressof(qv), q_rows,
             None if null_c else C.addressof(qo), None if null_cv else C.addressof(qv), c_rows, cutoff,
             None if null_out else C.addressof(out), c_rows if ld is None else ld)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case,kw,msg", [
    ("measure5", dict(measure=5), "measure 5 is not a measure of cdist"),
    ("measure6", dict(measure=6), "measure 6 is not a measure of cdist"),
    ("measure10", dict(measure=10), "measure 10 is not a measure of cdist"),
    ("measure16", dict(measure=16), "measure 16 is not a measure of cdist"),
    ("measure26", dict(measure=26), "measure 26 is not a measure of cdist"),
    ("measure-1", dict(measure=-1), "measure -1 is not a measure of cdist"),
    ("nan_cutoff", dict(cutoff=float("nan")), "score_cutoff is NaN"),
    ("short_ld", dict(c_rows=3, ld=2), "out_ld=2 is less than the 3 candidates of a row"),
    ("null_queries", dict(null_q=True), "NULL query buffer"),
    ("null_query_values", dict(null_qv=True), "NULL query buffer"),
    ("null_candidates", dict(null_c=True), "NULL candidate buffer"),
    ("null_candidate_values", dict(null_cv=True), "NULL candidate buffer"),
    ("null_output", dict(null_out=True), "NULL output buffer"),
    ("too_many_candidates", dict(c_rows=2 ** 32 - 1), "candidates (at most 2^32 - 2)"),
    ("too_many_queries", dict(q_rows=2 ** 32), "queries (at most 2^32 - 1)"),
])
def test_cdist_argument_errors_need_no_device(L, name, case, kw, msg):
    assert _call(L, name, **kw) == ERR_ARG
    text = L.strsim_last_error_message().decode()
    assert text.startswith(name + ": ") and msg in text
    if case.startswith("measure"):
        assert text.endswith("(the reference measures 0 .. 4, STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("measure", [0, 1, 2, 3, 4, 8, 14])
@pytest.mark.parametrize("kw", [dict(), dict(cutoff=0.5), dict(cutoff=1.5), dict(ld=9), dict(q_rows=0, null_q=True, null_qv=True, null_out=True),
                                dict(c_rows=0, null_c=True, null_cv=True, null_out=True)])
def test_cdist_null_context_is_checked_last(L, name, measure, kw):
    assert _call(L, name, measure=measure, **kw) == ERR_ARG
    assert "ctx is NULL" in L.strsim_last_error_message().decode()


def test_cdist_searches_keep_their_refusals(L):
    vp, u64 = C.c_void_p, C.c_uint64
    qo = (C.c_uint32 * 2)(0, 1)
    qv = (C.c_uint8 * 1)(97)
    out = (C.c_double * 8)()
    a = [C.addressof(qo), C.addressof(qv), 1, C.addressof(qo), C.addressof(qv), 1]
    for name, measure, msg in (("strsim_best_match_host", 8, "unknown measure 8"), ("strsim_nearest_host", 8, "has no distance"),
                               ("strsim_extract_host", 0, "is not a scorer of extract")):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, C.c_uint32] + ([C.c_uint32] if "nearest" in name else [C.c_double]) + [vp, vp]
        assert f(None, measure, *a, 1, 0, C.addressof(out), C.addressof(out)) == ERR_ARG
        assert msg in L.strsim_last_error_message().decode()


# ---- the Python surface -------------------------------------------------------------------------------------------------------

class _StubContext:
    """Context.cdist with the device replaced by the reference: records what it was asked for"""
    def __init__(self):
        self.calls = []

    def cdist(self, measure, qo, qv, co, cv, score_cutoff=None, out=None):
        self.calls.append((measure, len(qo) - 1, len(co) - 1, score_cutoff))
        raw_q, raw_c = bytes(qv), bytes(cv)
        Q = [raw_q[qo[i]:qo[i + 1]].decode() for i in range(len(qo) - 1)]
        Cs = [raw_c[co[j]:co[j + 1]].decode() for j in range(len(co) - 1)]
        return R.cdist("ratio" if measure == "indel" else measure, Q, Cs, score_cutoff)

    def default_process_host(self, off, val):
        raise AssertionError("no processor was asked for")


def test_cdist_python_surface():
    import strsim_amd
    from strsim_amd.context import Context
    assert "cdist" in strsim_amd.__all__ and "CDIST_MEASURES" in strsim_amd.__all__ and callable(strsim_amd.cdist)
    assert strsim_amd.CDIST_MEASURES == strsim_amd.MEASURES + ("ratio", "token_sort_ratio")
    assert callable(Context.cdist)
    for bad in ("osa", "partial_ratio", "token_set_ratio", "wratio", "cdist", 8, None):
        with pytest.raises(ValueError, match=r"no cdist by measure .*'ratio', 'token_sort_ratio'\)"):
            strsim_amd.cdist(bad, ["a"], ["b"])
    with pytest.raises(ValueError, match="unknown processor 'lower'"):
        strsim_amd.cdist("ratio", ["a"], ["b"], processor="lower")
    # the searches refuse what they refused
    with pytest.raises(ValueError, match="no best match"):
        strsim_amd.best_match("indel", ["a"], ["b"])
    with pytest.raises(ValueError, match="no extract by scorer"):
        strsim_amd.extract("jaro", ["a"], ["b"])


def test_cdist_python_alias_and_null_handling_with_a_stubbed_context():
    import strsim_amd
    E = lambda d, s: indel_ref.normalise(d, s, 0)
    Q = ["kitten", None, "abc"]
    Cs = [None, "sitting", "abd", None, "kitten"]
    stub = _StubContext()
    M = strsim_amd.cdist("ratio", Q, Cs, ctx=stub)
    assert stub.calls == [("indel", 3, 3, None)]  # the null candidates are not sent; the null query is, as ""
    assert M.shape == (3, 5) and M.dtype == np.float64
    assert np.isnan(M[1]).all() and np.isnan(M[:, 0]).all() and np.isnan(M[:, 3]).all()
    assert M[0, 4] == 1.0 and M[0, 1] == E(5, 13) and M[0, 2] == E(9, 9) and M[2, 2] == E(2, 6) and M[2, 1] == E(10, 10)
    assert R.same(strsim_amd.cdist("indel", Q, Cs, ctx=stub), M) and stub.calls[-1][0] == "indel"
    Z = strsim_amd.cdist("ratio", Q, Cs, score_cutoff=0.7, ctx=stub)
    assert stub.calls[-1] == ("indel", 3, 3, 0.7)
    assert Z[0, 4] == 1.0 and Z[0, 1] == 0.0 and np.isnan(Z[1]).all() and np.isnan(Z[0, 0])
    T = strsim_amd.cdist("token_sort_ratio", ["b a"], [None, "ab", "a  b"], ctx=stub)
    assert stub.calls[-1][0] == "token_sort_ratio" and np.isnan(T[0, 0]) and T[0, 2] == 1.0
    # nothing to score: the context is not called
    n = len(stub.calls)
    assert strsim_amd.cdist("jaro", [], ["a"], ctx=stub).shape == (0, 1)
    assert np.isnan(strsim_amd.cdist("jaro", ["a", "b"], [None], ctx=stub)).all()
    assert strsim_amd.cdist("jaro", ["a"], [], ctx=stub).shape == (1, 0) and len(stub.calls) == n


def test_cdist_polars_wrapper_source():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert '__all__ += ["cdist"]' in src
    assert 'def cdist(expr: IntoExpr, candidates: IntoExpr, measure: str = "ratio", score_cutoff: float | None = None) -> pl.Expr:' in src
    body = src[src.index("def cdist("):]
    for word in ("process.cdist", "List(Float64)", "/ 100", "is_elementwise=False", '"cdist_" + measure', "pl.lit(score_cutoff, dtype=pl.Float64)"):
        assert word in body, word


@pytest.mark.parametrize("m", PLUGIN)
def test_cdist_field_is_a_large_list_of_f64_named_after_first_input(m):
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    want = pa.large_list(pa.field("item", pa.float64()))
    assert arrow_host.field_plugin("cdist_" + m, ("queries", "cands")) == ("queries", want)
    assert arrow_host.field_plugin("cdist_" + m, ("q", "c", "score_cutoff")) == ("q", want)
