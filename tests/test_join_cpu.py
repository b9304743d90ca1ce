"""The threshold join without a GPU: the exported symbols and version, every argument error before any device, the Python surfaces
with the context stubbed (the capacity retry, null handling and index mapping, dedupe_pairs), the plugin's field functions, and the
host build of the rules the join kernels share with the host (strsim_join.h): a wave's count and fill sweeps replayed against brute
force, the sort network, the 64-bit scan and the split rule."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import indel_ref
import join_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "join_harness.cpp")
ERR_ARG = 2
INF = float("inf")
NAMES = ("strsim_join_device", "strsim_join_host")
PLUGIN = ("ratio", "token_sort_ratio")


def E(d, s):
    return indel_ref.normalise(d, s, 0)


CUTS = (-INF, 0.0, 0.5, math.nextafter(E(2, 6), 0.0), E(2, 6), math.nextafter(E(2, 6), 2.0), 1.0, 1.5)


@pytest.fixture(scope="module")
def L():
    import strsim_amd
    return strsim_amd.lib()  # (a library without strsim_join_device fails here: nothing is skipped)


def _build(out, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", CSRC, *flags, "-o", out, HARNESS])


@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="join_harness_")
    so = os.path.join(d.name, "libjoin_harness.so")
    _build(so, "-fPIC", "-shared")
    L = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    L.join_replay.restype = C.c_int
    L.join_replay.argtypes = [u64, u32, u32, u32, C.c_double, C.c_int, u32, C.c_int, C.POINTER(u64)]
    L.join_replay_all.restype = u32
    L.join_sort_check.restype = C.c_int
    L.join_sort_check.argtypes = [u64, u64]
    L.join_scan_check.restype = C.c_int
    L.join_scan_check.argtypes = [u64, u64, C.POINTER(u64)]
    L.join_splits_h.restype = u32
    L.join_splits_h.argtypes = [u64, u64, C.c_int]
    for name in ("join_sort_wave_max", "join_max_splits", "join_min_per_split", "join_wg_per_cu"):
        getattr(L, name).restype = u32
    L.join_map_shift_h.restype = u32
    L.join_map_shift_h.argtypes = [u64, u64, u32]
    L.join_map_words_h.restype = u64
    L.join_map_words_h.argtypes = [u64, u32, u32]
    L.join_pair_score.restype = C.c_double
    L.join_pair_score.argtypes = [u32, u32]
    yield L
    d.cleanup()


# ---- the rules of the sweep -----------------------------------------------------------------------------------------------------

def test_join_sweeps_replay_against_brute_force(H):
    # every cutoff of the list, with and without upper, 1 .. 3 splits, with and without an undersized segment, six frames each
    assert H.join_replay_all() == 0


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("upper", [0, 1])
def test_join_sweep_finds_every_hit_once_inside_its_segment(H, cut, upper):
    stats = (C.c_uint64 * 2)()
    for seed, nq, nc, maxlen, splits in ((1, 64, 300, 32, 1), (2, 64, 300, 32, 4), (3, 17, 129, 32, 3), (4, 64, 200, 5, 2), (5, 1, 90, 32, 2)):
        for under in (0, 1):
            assert H.join_replay(seed, nq, nc, maxlen, cut, upper, splits, under, stats) == 0, (seed, under)
        if cut <= 0.0 and not upper:
            assert stats[0] == nc and stats[1] == nq * nc  # no cutoff: every candidate is visited, every pair is a hit
        if cut > 1.0:
            assert stats[0] == 0 and stats[1] == 0         # nothing is admissible: no sweep


def test_join_pruning_skips_candidates(H):
    # a wave of one-length-apart queries under a high cutoff visits only the lengths around its own
    stats = (C.c_uint64 * 2)()
    assert H.join_replay(11, 64, 500, 32, 0.9, 0, 1, 0, stats) == 0
    dense = stats[0]
    assert H.join_replay(11, 64, 500, 5, 0.9, 0, 1, 0, stats) == 0  # lengths 0 .. 5 only: the window is most of the range
    assert stats[0] <= 500 and dense <= 500
    assert H.join_replay(12, 1, 500, 32, 0.9, 0, 1, 0, stats) == 0  # one query: its window at 0.9 is a few lengths wide
    assert 0 < stats[0] < 250
    assert H.join_replay(12, 1, 500, 32, 1.0, 0, 2, 0, stats) == 0  # at 1.0: its own length alone
    assert stats[0] < 60


def test_join_hit_is_the_f64_comparison_at_the_neighbours_of_a_score(H):
    e = H.join_pair_score(2, 6)
    assert e == E(2, 6)
    stats = (C.c_uint64 * 2)()
    n = []
    for cut in (math.nextafter(e, 0.0), e, math.nextafter(e, 2.0)):
        assert H.join_replay(21, 64, 400, 6, cut, 0, 2, 0, stats) == 0
        n.append(stats[1])
    assert n[0] == n[1] > n[2]  # pairs that score exactly E(2, 6) exist in the frame and leave at the next double


# ---- the sort network, the scan and the split rule ------------------------------------------------------------------------------

def test_join_sort_network_equals_std_sort_at_every_length(H):
    tier = H.join_sort_wave_max()
    assert tier == 512
    for n in list(range(0, 131)) + [tier - 1, tier, tier + 1, 2 * tier, 3 * tier, 4097, 5000]:
        for seed in (1, 2):
            assert H.join_sort_check(n, seed) == 0, n


def test_join_scan_is_exact_beyond_32_bits(H):
    total = C.c_uint64()
    for n in (0, 1, 7, 255, 256, 2047, 2048, 2049, 4096, 4097, 100000, 600000):
        assert H.join_scan_check(n, 1 << 31, C.byref(total)) == 0, n
        assert total.value == sum((1 << 31) + (x & 7) for x in range(n))
    assert total.value > 2 ** 32
    assert H.join_scan_check(5000, 2 ** 40, C.byref(total)) == 0 and total.value > 2 ** 52


def test_join_splits_fill_the_device_and_keep_the_counts_small(H):
    cap, per, wgs = H.join_max_splits(), H.join_min_per_split(), H.join_wg_per_cu()
    assert (cap, per, wgs) == (64, 64, 16)

    def want(nq, nc, cu=256):
        qblocks = -(-nq // 256)
        return max(1, min(-(-wgs * cu // qblocks), -(-nc // per), cap))
    for nq, nc in ((5, 3000), (257, 129), (300, 700), (20000, 10000), (200000, 200000), (10 ** 6, 10 ** 6), (1, 1), (1, 2 ** 32 - 2), (2 ** 32 - 1, 5)):
        assert H.join_splits_h(nq, nc, 256) == want(nq, nc), (nq, nc)
    assert H.join_splits_h(257, 129, 256) == 3 and H.join_splits_h(257, 129, 64) == 3  # few candidates: 64 per split at least
    assert H.join_splits_h(20000, 10000, 256) == 52 and H.join_splits_h(200000, 200000, 256) == 6
    assert H.join_splits_h(2 ** 21, 10 ** 6, 256) == 1                                  # enough query workgroups: no split
    assert H.join_splits_h(7, 10 ** 9, 0) == 64
    # the counts: (splits + 1) words per query
    for nq in (1, 1000, 20000, 200000, 2 ** 20, 2 ** 32 - 1):
        s = H.join_splits_h(nq, 2 ** 32 - 2, 256)
        assert s == 1 or (s + 1) * nq <= 2 * 256 * (wgs * 256 + nq // 256 + 1)


def test_join_hit_map_stays_within_its_budget(H):
    # one bit per (wave, candidate) while that fits 256 MB, then one per group of 2, 4, .. candidates; every slice has words of its own
    budget = 256 << 20
    assert H.join_map_shift_h(20000, 10000, 52) == 0 and H.join_map_shift_h(200000, 200000, 6) == 0
    assert H.join_map_words_h(10000, 52, 0) == 10000 // 32 + 34 * 52 + 2
    for nq, nc in ((20000, 10000), (200000, 200000), (10 ** 6, 10 ** 6), (10 ** 7, 10 ** 6), (2 ** 25, 2 ** 32 - 2)):
        splits = H.join_splits_h(nq, nc, 256)
        shift = H.join_map_shift_h(nq, nc, splits)
        waves = -(-nq // 64)
        assert waves * H.join_map_words_h(nc, splits, shift) * 4 <= budget or shift == 31
        assert shift == 0 or waves * H.join_map_words_h(nc, splits, shift - 1) * 4 > budget
    assert H.join_map_shift_h(10 ** 6, 10 ** 6, 1) == 3


def test_join_harness_stands_alone(tmp_path):
    # the same checks as a program of its own (the form that is run under the sanitizers)
    exe = str(tmp_path / "join_harness")
    _build(exe, "-DJOIN_HARNESS_MAIN")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 replays failed, 0 sorts differ, 0 scans differ, totals beyond 2^32" in out.stdout


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_join_keeps_abi_version_1_7(L):
    assert L.strsim_abi_version() == 0x00010007
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    assert re.search(r"#define STRSIM_ABI_VERSION 0x00010007u", hdr) and "#define STRSIM_JOIN_UPPER 1u" in hdr
    for name in NAMES:
        assert re.search(r"STRSIM_API int " + name + r"\(strsim_ctx_t \*ctx, int scorer,", hdr)


def test_join_symbols_are_exported(L):
    hdr = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    for name in NAMES:
        assert getattr(L, name) is not None
    for m in PLUGIN:
        assert getattr(L, "_polars_plugin_join_" + m) is not None and getattr(L, "_polars_plugin_field_join_" + m) is not None
        assert "POLARS_PLUGIN_DECLARE(join_%s)" % m in hdr


def test_join_leaves_measure_supported_alone(L):
    for m in (8, 14):
        assert L.strsim_measure_supported(m, 1) == 0 and L.strsim_measure_supported(m, 0) == 1
    for m in range(-1, 18):
        assert L.strsim_measure_supported(m, 3) == 0


def _call(L, name, scorer=8, q_rows=1, c_rows=1, cutoff=-INF, flags=0, capacity=4, null=()):
    qo = (C.c_uint32 * 2)(0, 1)
    qv = (C.c_uint8 * 1)(97)
    indptr = (C.c_uint64 * 4)()
    index = (C.c_uint32 * 4)()
    score = (C.c_double * 4)()
    nnz = C.c_uint64(77)
    arg = lambda key, obj: None if key in null else C.addressof(obj)
    f = getattr(L, name)
    return f(None, scorer, arg("q_off", qo), arg("q_val", qv), q_rows, arg("c_off", qo), arg("c_val", qv), c_rows, cutoff, flags, capacity,
             arg("indptr", indptr), arg("index", index), arg("score", score), C.cast(arg("nnz", nnz), C.POINTER(C.c_uint64)))


ARG_ERRORS = [
    ("scorer0", dict(scorer=0), "scorer 0 is not a scorer of join (STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)"),
    ("scorer10", dict(scorer=10), "scorer 10 is not a scorer of join (STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)"),
    ("scorer16", dict(scorer=16), "scorer 16 is not a scorer of join (STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)"),
    ("scorer-1", dict(scorer=-1), "scorer -1 is not a scorer of join (STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)"),
    ("nan_cutoff", dict(cutoff=float("nan")), "score_cutoff is NaN"),
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
    ("nan_before_flags", dict(cutoff=float("nan"), flags=8), "score_cutoff is NaN"),
    ("scorer_before_nan", dict(scorer=3, cutoff=float("nan")), "scorer 3 is not a scorer of join (STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)"),
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case,kw,msg", ARG_ERRORS)
def test_join_argument_errors_need_no_device(L, name, case, kw, msg):
    assert _call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": " + msg


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("scorer", [8, 14])
@pytest.mark.parametrize("kw", [dict(), dict(cutoff=0.5), dict(cutoff=1.5), dict(flags=1), dict(capacity=0, null=("index", "score")),
                                dict(q_rows=0, null=("q_off", "q_val")), dict(c_rows=0, null=("c_off", "c_val"))])
def test_join_null_context_is_checked_last(L, name, scorer, kw):
    assert _call(L, name, scorer=scorer, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": ctx is NULL"


# ---- the Python surfaces --------------------------------------------------------------------------------------------------------

def _decode(off, val):
    raw = bytes(val)
    return [raw[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


class _StubLibContext:
    """strsim_amd.join above Context.join, the device replaced by the reference: records what it was asked for"""
    def __init__(self):
        self.calls = []

    def join(self, scorer, qo, qv, co, cv, score_cutoff=None, upper=False):
        Q, Cs = _decode(qo, qv), _decode(co, cv)
        self.calls.append((scorer, Q, Cs, score_cutoff, upper))
        return R.join("ratio" if scorer == "indel" else scorer, Q, Cs, score_cutoff, upper)

    def default_process_host(self, off, val):
        raise AssertionError("no processor was asked for")


def test_join_python_surface():
    import strsim_amd
    from strsim_amd.context import Context
    for name in ("join", "dedupe_pairs", "JOIN_SCORERS"):
        assert name in strsim_amd.__all__
    assert strsim_amd.JOIN_SCORERS == ("ratio", "token_sort_ratio") and callable(Context.join)
    for bad in ("jaro", "levenshtein", "wratio", 8, None):
        with pytest.raises(ValueError, match=r"no join by scorer .*\('ratio', 'token_sort_ratio'\)"):
            strsim_amd.join(bad, ["a"], ["b"], 0.5)
    with pytest.raises(ValueError, match="unknown processor 'lower'"):
        strsim_amd.join("ratio", ["a"], ["b"], 0.5, processor="lower")


def test_join_null_handling_and_index_mapping_with_a_stubbed_context():
    import strsim_amd
    Q = ["kitten", None, "abc", ""]
    Cs = [None, "sitting", "abd", None, "kitten", ""]
    stub = _StubLibContext()
    indptr, index, score = strsim_amd.join("ratio", Q, Cs, 0.6, ctx=stub)
    # the null candidates are not sent; the null query is, as "", and its row is emptied afterwards
    assert stub.calls == [("indel", ["kitten", "", "abc", ""], ["sitting", "abd", "kitten", ""], 0.6, False)]
    assert indptr.dtype == np.int64 and index.dtype == np.int64 and score.dtype == np.float64
    assert indptr.tolist() == [0, 2, 2, 3, 4] and index.tolist() == [1, 4, 2, 5]
    assert score.tolist() == [E(5, 13), 1.0, E(2, 6), 1.0]
    # "indel" is an alias, None reports every pair of the non-null rows
    indptr, index, score = strsim_amd.join("indel", Q, Cs, None, ctx=stub)
    assert stub.calls[-1][3] is None and indptr.tolist() == [0, 4, 4, 8, 12] and index.tolist() == [1, 2, 4, 5] * 3
    T = strsim_amd.join("token_sort_ratio", ["b a"], [None, "ab", "a  b"], 1.0, ctx=stub)
    assert stub.calls[-1][0] == "token_sort_ratio" and T[0].tolist() == [0, 1] and T[1].tolist() == [2] and T[2].tolist() == [1.0]
    # empty sides
    assert strsim_amd.join("ratio", [], ["a"], 0.5, ctx=stub)[0].tolist() == [0]
    assert strsim_amd.join("ratio", ["a", None], [], 0.5, ctx=stub)[0].tolist() == [0, 0, 0]
    assert strsim_amd.join("ratio", ["a"], [None, None], None, ctx=stub)[0].tolist() == [0, 0]


def test_dedupe_pairs_with_a_stubbed_context():
    import strsim_amd
    col = ["anna", "bob", None, "anna", "anne", "bob", None, ""]
    stub = _StubLibContext()
    i, j, s = strsim_amd.dedupe_pairs("ratio", col, 0.7, ctx=stub)
    # upper compares positions: the nulls keep theirs (as empty strings) and their pairs are dropped -- (2, 6), (2, 7), (6, 7)
    assert stub.calls == [("indel", [c or "" for c in col], [c or "" for c in col], 0.7, True)]
    assert list(zip(i.tolist(), j.tolist())) == [(0, 3), (0, 4), (1, 5), (3, 4)]
    assert s.tolist() == [1.0, E(2, 8), 1.0, E(2, 8)] and i.dtype == j.dtype == np.int64
    i, j, s = strsim_amd.dedupe_pairs("ratio", [], 0.7, ctx=stub)
    assert i.size == j.size == s.size == 0
    i, j, s = strsim_amd.dedupe_pairs("ratio", ["a", "a", "a"], None, ctx=stub)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (0, 2), (1, 2)]


class _FakeLib:
    """strsim_join_host as Context.join calls it: the capacity protocol over a fixed result"""
    def __init__(self, result):
        self.result = result
        self.capacities = []

    def strsim_join_host(self, h, scorer, qo, qv, nq, co, cv, nc, cut, flags, capacity, indptr, index, score, nnz):
        ip, ix, sc = self.result
        self.capacities.append((capacity, index is None, flags, cut))
        C.memmove(indptr, ip.ctypes.data, ip.nbytes)
        C.cast(nnz, C.POINTER(C.c_uint64))[0] = ix.size
        if ix.size <= capacity and ix.size:
            C.memmove(index, ix.ctypes.data, ix.nbytes)
            C.memmove(score, sc.ctypes.data, sc.nbytes)
        return 0


def test_context_join_retries_once_with_the_exact_size(monkeypatch):
    import strsim_amd
    from strsim_amd import context
    Q, Cs = ["ab", "abc", "b"], ["ab", "abc", "abd", "b"]
    exp = R.join("ratio", Q, Cs, 0.5)
    fake = _FakeLib(exp)
    monkeypatch.setattr(context, "lib", lambda: fake)
    ctx = context.Context.__new__(context.Context)
    ctx._h = None
    cols = (*strsim_amd.pack_strings(Q), *strsim_amd.pack_strings(Cs))
    n = exp[1].size
    assert n > 3
    assert R.same(ctx.join("indel", *cols, 0.5, capacity=3), exp) and [c[0] for c in fake.capacities] == [3, n]
    fake.capacities.clear()
    assert R.same(ctx.join("indel", *cols, 0.5), exp) and [c[0] for c in fake.capacities] == [4 * 3 + 1024]  # the guess holds: one call
    fake.capacities.clear()
    assert R.same(ctx.join("indel", *cols, 0.5, upper=True, capacity=n), exp) and fake.capacities == [(n, False, 1, 0.5)]
    fake.capacities.clear()
    assert np.array_equal(ctx.join("indel", *cols, None, count_only=True), exp[0]) and fake.capacities == [(0, True, 0, -INF)]
    fake.capacities.clear()
    got = ctx.join("indel", *cols, 0.5, capacity=0)  # NULL outputs with capacity 0, then the exact size
    assert R.same(got, exp) and fake.capacities == [(0, True, 0, 0.5), (n, False, 0, 0.5)]


def test_join_polars_wrapper_source():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert '__all__ += ["join"]' in src
    assert 'def join(expr: IntoExpr, candidates: IntoExpr, scorer: str = "ratio", score_cutoff: float | None = None) -> pl.Expr:' in src
    body = src[src.index("def join("):]
    for word in ("List(Struct{index: UInt32, score: Float64})", "/ 100", "is_elementwise=False", '"join_" + scorer', "pl.lit(score_cutoff, dtype=pl.Float64)"):
        assert word in body, word


@pytest.mark.parametrize("m", PLUGIN)
def test_join_field_is_a_large_list_of_structs_named_after_first_input(m):
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    want = pa.large_list(pa.field("item", pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])))
    assert arrow_host.field_plugin("join_" + m, ("queries", "cands")) == ("queries", want)
    assert arrow_host.field_plugin("join_" + m, ("q", "c", "score_cutoff")) == ("q", want)
