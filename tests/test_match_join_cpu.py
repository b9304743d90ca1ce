"""match_join (the threshold join by the five reference measures) without a GPU: the exported symbols, every argument error before
any device, the pruning bound checked with the library's own epilogues over every integer tuple, the need mask, a wave's count and
fill sweeps replayed against brute force (strsim_match_join.h compiled by g++), and the Python surfaces with the context stubbed."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import match_join_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "match_join_harness.cpp")
ERR_ARG = 2
INF = float("inf")
NAMES = ("strsim_match_join_device", "strsim_match_join_host")
JOIN_NAMES = ("strsim_join_device", "strsim_join_host")
MEASURES = R.MEASURES


@pytest.fixture(scope="module")
def L():
    import strsim_amd
    return strsim_amd.lib()  # (a library without strsim_match_join_device fails here: nothing is skipped)


def _build(out, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", CSRC, *flags, "-o", out, HARNESS])


@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="match_join_harness_")
    so = os.path.join(d.name, "libmatch_join_harness.so")
    _build(so, "-fPIC", "-shared")
    lib = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    lib.mj_ub.restype = C.c_double
    lib.mj_ub.argtypes = [C.c_int, u32, u32]
    lib.mj_bound_check.restype = u32
    lib.mj_bound_check.argtypes = [C.c_int]
    lib.mj_need_mask.restype = C.c_int
    lib.mj_need_mask.argtypes = [C.c_int, C.c_double, C.POINTER(u64)]
    lib.mj_replay.restype = C.c_int
    lib.mj_replay.argtypes = [u64, C.c_int, u32, u32, u32, C.c_double, C.c_int, u32, C.c_int, u32, C.POINTER(u64)]
    lib.mj_replay_all.restype = u32
    lib.mj_lengths.restype = u32
    lib.mj_need_bytes.restype = u32
    yield lib
    d.cleanup()


def _cuts(H, m):
    """-inf, 0, 0.5, 0.8, 1.0, 1.5, and the bound of lengths (7, 9) with its two f64 neighbours"""
    e = H.mj_ub(m, 7, 9)
    return (-INF, 0.0, 0.5, 0.8, 1.0, 1.5, math.nextafter(e, 0.0), e, math.nextafter(e, 2.0))


# ---- the symbols ----------------------------------------------------------------------------------------------------------------

def test_match_join_symbols_are_exported(L):
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    plug = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    for name in NAMES:
        assert getattr(L, name) is not None
        assert "STRSIM_API int " + name + "(strsim_ctx_t *ctx, int measure," in hdr
    for m in MEASURES:
        assert getattr(L, "_polars_plugin_match_join_" + m) is not None and getattr(L, "_polars_plugin_field_match_join_" + m) is not None
        assert "POLARS_PLUGIN_DECLARE(match_join_%s)" % m in plug


def test_match_join_leaves_the_abi_version_and_measure_supported_alone(L):
    assert L.strsim_abi_version() == 0x00010007
    for m in range(-1, 28):
        assert L.strsim_measure_supported(m, 3) == 0


# ---- the bound and the need mask ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", range(5))
def test_match_join_bound_is_the_maximum_over_every_tuple(H, m):
    # no tuple the kernel can produce scores above match_join_ub at any pair of lengths 0 .. 32, and some tuple attains it
    assert H.mj_lengths() == 33 and H.mj_need_bytes() == 264
    assert H.mj_bound_check(m) == 0


def test_match_join_bound_values(H):
    for m in range(5):
        assert H.mj_ub(m, 0, 0) == 1.0 and H.mj_ub(m, 0, 5) == 0.0 and H.mj_ub(m, 32, 0) == 0.0
        for l in range(1, 33):
            assert H.mj_ub(m, l, l) == 1.0
        for lq in range(33):
            for lc in range(33):
                assert H.mj_ub(m, lq, lc) == H.mj_ub(m, lc, lq)
    assert H.mj_ub(0, 7, 9) == 1.0 - 2.0 / 9.0
    assert H.mj_ub(1, 7, 9) == (7.0 / 7.0 + 7.0 / 9.0 + 7.0 / 7.0) / 3.0
    j = H.mj_ub(1, 7, 9)
    assert H.mj_ub(2, 7, 9) == j + (4.0 * 0.1 * (1.0 - j))
    assert H.mj_ub(3, 7, 9) == 7.0 / 9.0 and H.mj_ub(4, 7, 9) == 14.0 / 16.0
    j = H.mj_ub(1, 1, 32)  # (1 + 1 / 32 + 1) / 3, below the 0.7 gate: no boost
    assert j <= 0.7 and H.mj_ub(2, 1, 32) == j


@pytest.mark.parametrize("m", range(5))
def test_match_join_need_mask_is_the_direct_comparison(H, m):
    w = (C.c_uint64 * 33)()
    for cut in _cuts(H, m):
        any_bit = H.mj_need_mask(m, cut, w)
        for lq in range(33):
            want = sum(1 << lc for lc in range(33) if H.mj_ub(m, lq, lc) >= cut)
            assert w[lq] == want, (cut, lq)
        assert any_bit == (1 if cut <= 1.0 else 0)
    e = H.mj_ub(m, 7, 9)
    H.mj_need_mask(m, e, w)
    assert (w[7] >> 9) & 1 and (w[9] >> 7) & 1
    H.mj_need_mask(m, math.nextafter(e, 2.0), w)
    assert not (w[7] >> 9) & 1 and not (w[9] >> 7) & 1


# ---- the rules of the sweep -----------------------------------------------------------------------------------------------------

def test_match_join_sweeps_replay_against_brute_force(H):
    # five measures, every cutoff of the list, with and without upper, 1 .. 3 splits, hit-map groups of 1, 2 and 4, with and without
    # an undersized segment, four frames each
    assert H.mj_replay_all() == 0


@pytest.mark.parametrize("m", range(5))
@pytest.mark.parametrize("upper", [0, 1])
def test_match_join_sweep_finds_every_hit_once_inside_its_segment(H, m, upper):
    stats = (C.c_uint64 * 3)()
    for cut in _cuts(H, m):
        for seed, nq, nc, maxlen, splits, shift in ((1, 64, 300, 32, 1, 0), (2, 64, 300, 32, 3, 1), (3, 17, 129, 32, 3, 2), (4, 64, 200, 5, 2, 0),
                                                    (5, 1, 90, 32, 2, 1)):
            for under in (0, 1):
                assert H.mj_replay(seed, m, nq, nc, maxlen, cut, upper, splits, under, shift, stats) == 0, (cut, seed, under)
            if cut <= 0.0 and not upper:
                assert stats[0] == nc and stats[1] == nq * nc  # no cutoff: every candidate is visited, every pair is a hit
            if cut > 1.0:
                assert stats[0] == 0 and stats[1] == 0         # nothing is admissible: no sweep


def test_match_join_pruning_skips_lengths(H):
    stats = (C.c_uint64 * 3)()
    w = (C.c_uint64 * 33)()
    for m in range(5):
        # one query: the sweep visits exactly the lengths of its own word, a strict subset at 0.8 for every measure
        assert H.mj_replay(12, m, 1, 500, 32, 0.8, 0, 2, 0, 0, stats) == 0
        H.mj_need_mask(m, 0.8, w)
        assert stats[2] in set(w) and 0 < bin(stats[2]).count("1") < 33 and stats[0] < 500
        assert H.mj_replay(12, m, 1, 500, 32, 1.0, 0, 2, 0, 0, stats) == 0  # at 1.0: its own length alone
        assert bin(stats[2]).count("1") == 1 and stats[0] < 60


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def _call(L, name, measure=2, q_rows=1, c_rows=1, cutoff=-INF, flags=0, capacity=4, null=()):
    qo = (C.c_uint32 * 2)(0, 1)
    qv = (C.c_uint8 * 1)(97)
    indptr = (C.c_uint64 * 4)()
    index = (C.c_uint32 * 4)()
    score = (C.c_double * 4)()
    nnz = C.c_uint64(77)
    arg = lambda key, obj: None if key in null else C.addressof(obj)
    f = getattr(L, name)
    return f(None, measure, arg("q_off", qo), arg("q_val", qv), q_rows, arg("c_off", qo), arg("c_val", qv), c_rows, cutoff, flags, capacity,
             arg("indptr", indptr), arg("index", index), arg("score", score), C.cast(arg("nnz", nnz), C.POINTER(C.c_uint64)))


NOT_A_MEASURE = "measure %d is not a measure of match_join (the reference measures 0 .. 4)"
ARG_ERRORS = [
    ("measure5", dict(measure=5), NOT_A_MEASURE % 5),
    ("measure8", dict(measure=8), NOT_A_MEASURE % 8),
    ("measure14", dict(measure=14), NOT_A_MEASURE % 14),
    ("measure-1", dict(measure=-1), NOT_A_MEASURE % -1),
    ("nan_cutoff", dict(cutoff=float("nan")), "min_score is NaN"),
    ("flags2", dict(flags=2), "unknown flags 0x2 (STRSIM_JOIN_UPPER = 1)"),
    ("flags3", dict(flags=3), "unknown flags 0x3 (STRSIM_JOIN_UPPER = 1)"),
    ("too_many_queries", dict(q_rows=2 ** 32), "4294967296 queries (at most 2^32 - 1)"),
    ("too_many_candidates", dict(c_rows=2 ** 32 - 1), "4294967295 candidates (at most 2^32 - 2)"),
    ("null_queries", dict(null=("q_off",)), "NULL query buffer"),
    ("null_query_values", dict(null=("q_val",)), "NULL query buffer"),
    ("null_candidates", dict(null=("c_off",)), "NULL candidate buffer"),
    ("null_candidate_values", dict(null=("c_val",)), "NULL candidate buffer"),
    ("null_nnz", dict(null=("nnz",)), "out_nnz is NULL"),
    ("null_indptr", dict(null=("indptr",)), "out_indptr is NULL"),
    ("null_index", dict(null=("index",)), "capacity=4 with a NULL output buffer"),
    ("null_score", dict(null=("score",)), "capacity=4 with a NULL output buffer"),
    ("nan_before_flags", dict(cutoff=float("nan"), flags=8), "min_score is NaN"),
    ("measure_before_nan", dict(measure=9, cutoff=float("nan")), NOT_A_MEASURE % 9),
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case,kw,msg", ARG_ERRORS)
def test_match_join_argument_errors_need_no_device(L, name, case, kw, msg):
    assert _call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": " + msg


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("measure", range(5))
@pytest.mark.parametrize("kw", [dict(), dict(cutoff=0.5), dict(cutoff=1.5), dict(flags=1), dict(capacity=0, null=("index", "score")),
                                dict(q_rows=0, null=("q_off", "q_val")), dict(c_rows=0, null=("c_off", "c_val"))])
def test_match_join_null_context_is_checked_last(L, name, measure, kw):
    assert _call(L, name, measure=measure, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": ctx is NULL"


@pytest.mark.parametrize("name", JOIN_NAMES)
def test_join_still_refuses_the_reference_measures_in_its_own_words(L, name):
    for m in range(5):
        assert _call(L, name, measure=m) == ERR_ARG
        assert L.strsim_last_error_message().decode() == name + ": scorer %d is not a scorer of join (STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)" % m
    assert _call(L, name, measure=8, cutoff=float("nan")) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": score_cutoff is NaN"
    assert _call(L, name, measure=8) == ERR_ARG and L.strsim_last_error_message().decode() == name + ": ctx is NULL"


# ---- the Python surfaces --------------------------------------------------------------------------------------------------------

def _decode(off, val):
    raw = bytes(val)
    return [raw[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


class _StubContext:
    """strsim_amd.match_join above Context.match_join, the device replaced by the reference: records what it was asked for"""
    def __init__(self):
        self.calls = []

    def match_join(self, measure, qo, qv, co, cv, min_score=None, upper=False):
        Q, Cs = _decode(qo, qv), _decode(co, cv)
        self.calls.append((measure, Q, Cs, min_score, upper))
        return R.join(measure, Q, Cs, min_score, upper)

    def join(self, *a, **k):
        raise AssertionError("match_join goes through Context.match_join")

    def default_process_host(self, off, val):
        raise AssertionError("no processor was asked for")


def test_match_join_python_surface():
    import strsim_amd
    from strsim_amd.context import Context
    for name in ("match_join", "match_dedupe_pairs", "MATCH_JOIN_MEASURES"):
        assert name in strsim_amd.__all__
    assert strsim_amd.MATCH_JOIN_MEASURES == strsim_amd.MEASURES == MEASURES and callable(Context.match_join)
    assert strsim_amd.JOIN_SCORERS == ("ratio", "token_sort_ratio")
    for bad in ("ratio", "indel", "token_sort_ratio", "osa", 2, None):
        with pytest.raises(ValueError, match=r"no match_join by measure .*\(one of \('levenshtein', 'jaro', 'jaro_winkler', 'jaccard', 'sorensen_dice'\)\)"):
            strsim_amd.match_join(bad, ["a"], ["b"], 0.5)
    with pytest.raises(ValueError, match="unknown processor 'lower'"):
        strsim_amd.match_join("jaro", ["a"], ["b"], 0.5, processor="lower")


def test_match_join_null_handling_and_index_mapping_with_a_stubbed_context():
    import strsim_amd
    Q = ["kitten", None, "abc", ""]
    Cs = [None, "sitting", "abd", None, "kitten", ""]
    stub = _StubContext()
    indptr, index, score = strsim_amd.match_join("levenshtein", Q, Cs, 0.5, ctx=stub)
    # the null candidates are not sent; the null query is, as "", and its row is emptied afterwards
    assert stub.calls == [("levenshtein", ["kitten", "", "abc", ""], ["sitting", "abd", "kitten", ""], 0.5, False)]
    assert indptr.dtype == np.int64 and index.dtype == np.int64 and score.dtype == np.float64
    assert indptr.tolist() == [0, 2, 2, 3, 4] and index.tolist() == [1, 4, 2, 5]
    assert score.tolist() == [1.0 - 3.0 / 7.0, 1.0, 1.0 - 1.0 / 3.0, 1.0]
    # None reports every pair of the non-null rows
    indptr, index, score = strsim_amd.match_join("jaro_winkler", Q, Cs, None, ctx=stub)
    assert stub.calls[-1][0] == "jaro_winkler" and stub.calls[-1][3] is None
    assert indptr.tolist() == [0, 4, 4, 8, 12] and index.tolist() == [1, 2, 4, 5] * 3
    # empty sides
    assert strsim_amd.match_join("jaro", [], ["a"], 0.5, ctx=stub)[0].tolist() == [0]
    assert strsim_amd.match_join("jaro", ["a", None], [], 0.5, ctx=stub)[0].tolist() == [0, 0, 0]
    assert strsim_amd.match_join("jaccard", ["a"], [None, None], None, ctx=stub)[0].tolist() == [0, 0]


def test_match_dedupe_pairs_with_a_stubbed_context():
    import strsim_amd
    col = ["anna", "bob", None, "anna", "anne", "bob", None, ""]
    stub = _StubContext()
    i, j, s = strsim_amd.match_dedupe_pairs("levenshtein", col, 0.7, ctx=stub)
    # upper compares positions: the nulls keep theirs (as empty strings) and their pairs are dropped -- (2, 6), (2, 7), (6, 7)
    assert stub.calls == [("levenshtein", [c or "" for c in col], [c or "" for c in col], 0.7, True)]
    assert list(zip(i.tolist(), j.tolist())) == [(0, 3), (0, 4), (1, 5), (3, 4)]
    assert s.tolist() == [1.0, 0.75, 1.0, 0.75] and i.dtype == j.dtype == np.int64
    i, j, s = strsim_amd.match_dedupe_pairs("jaro", [], 0.7, ctx=stub)
    assert i.size == j.size == s.size == 0
    i, j, s = strsim_amd.match_dedupe_pairs("sorensen_dice", ["a", "a", "a"], None, ctx=stub)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (0, 2), (1, 2)]


class _FakeLib:
    """strsim_match_join_host as Context.match_join calls it: the capacity protocol over a fixed result"""
    def __init__(self, result):
        self.result = result
        self.capacities = []

    def strsim_match_join_host(self, h, measure, qo, qv, nq, co, cv, nc, cut, flags, capacity, indptr, index, score, nnz):
        ip, ix, sc = self.result
        self.capacities.append((capacity, index is None, flags, cut, measure))
        C.memmove(indptr, ip.ctypes.data, ip.nbytes)
        C.cast(nnz, C.POINTER(C.c_uint64))[0] = ix.size
        if ix.size <= capacity and ix.size:
            C.memmove(index, ix.ctypes.data, ix.nbytes)
            C.memmove(score, sc.ctypes.data, sc.nbytes)
        return 0


def test_context_match_join_retries_once_with_the_exact_size(monkeypatch):
    import strsim_amd
    from strsim_amd import context
    Q, Cs = ["ab", "abc", "b"], ["ab", "abc", "abd", "b"]
    exp = R.join("jaro_winkler", Q, Cs, 0.5)
    fake = _FakeLib(exp)
    monkeypatch.setattr(context, "lib", lambda: fake)
    ctx = context.Context.__new__(context.Context)
    ctx._h = None
    cols = (*strsim_amd.pack_strings(Q), *strsim_amd.pack_strings(Cs))
    n = exp[1].size
    assert n > 3
    assert R.same(ctx.match_join("jaro_winkler", *cols, 0.5, capacity=3), exp) and [c[0] for c in fake.capacities] == [3, n]
    fake.capacities.clear()
    assert R.same(ctx.match_join("jaro_winkler", *cols, 0.5), exp) and [c[0] for c in fake.capacities] == [4 * 3 + 1024]  # the guess holds
    fake.capacities.clear()
    assert R.same(ctx.match_join("jaro_winkler", *cols, 0.5, upper=True, capacity=n), exp) and fake.capacities == [(n, False, 1, 0.5, 2)]
    fake.capacities.clear()
    assert np.array_equal(ctx.match_join("jaro_winkler", *cols, None, count_only=True), exp[0]) and fake.capacities == [(0, True, 0, -INF, 2)]
    fake.capacities.clear()
    got = ctx.match_join("jaro_winkler", *cols, 0.5, capacity=0)  # NULL outputs with capacity 0, then the exact size
    assert R.same(got, exp) and fake.capacities == [(0, True, 0, 0.5, 2), (n, False, 0, 0.5, 2)]


def test_match_join_polars_wrapper_source():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert '__all__ += ["match_join"]' in src
    assert 'def match_join(expr: IntoExpr, candidates: IntoExpr, measure: str = "jaro_winkler", min_score: float | None = None) -> pl.Expr:' in src
    body = src[src.index("def match_join("):]
    for word in ("List(Struct{index: UInt32, score: Float64})", "is_elementwise=False", '"match_join_" + measure', "pl.lit(min_score, dtype=pl.Float64)"):
        assert word in body, word


@pytest.mark.parametrize("m", MEASURES)
def test_match_join_field_is_a_large_list_of_structs_named_after_first_input(m):
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    want = pa.large_list(pa.field("item", pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])))
    assert arrow_host.field_plugin("match_join_" + m, ("queries", "cands")) == ("queries", want)
    assert arrow_host.field_plugin("match_join_" + m, ("q", "c", "min_score")) == ("q", want)


def test_match_join_harness_stands_alone(tmp_path):
    # the same checks as a program of its own (the form that is run under the sanitizers)
    exe = str(tmp_path / "match_join_harness")
    _build(exe, "-DMATCH_JOIN_HARNESS_MAIN")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 length pairs off their bound, 0 mask bits differ, 0 replays failed" in out.stdout
