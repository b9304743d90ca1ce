"""qgram_join / qgram_cluster (the threshold join by q-gram similarity) without a GPU: the exported symbols, every argument error of
the four entry points before any device and the order of the checks, the pruning bound checked with the library's own qgram_score
over every admissible tuple, the need mask, the uniform-text scoring call against brute force, a wave's count and fill sweeps
replayed (strsim_qgram_join.h compiled by g++), the reference model against hand-written answers, and the Python surfaces with the
context stubbed."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import qgram_join_ref as R
import qgram_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "qgram_join_harness.cpp")
ERR_ARG = 2
INF = float("inf")
JOIN_NAMES = ("strsim_qgram_join_device", "strsim_qgram_join_host")
CLUSTER_NAMES = ("strsim_qgram_cluster_device", "strsim_qgram_cluster_host")
KINDS = R.KINDS
MODES = [(k, q, s) for k in range(4) for q in (1, 2, 3) for s in (0, 1)]


@pytest.fixture(scope="module")
def L():
    import strsim_amd
    return strsim_amd.lib()  # (a library without strsim_qgram_join_device fails here: nothing is skipped)


def _build(out, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", CSRC, *flags, "-o", out, HARNESS])


@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="qgram_join_harness_")
    so = os.path.join(d.name, "libqgram_join_harness.so")
    _build(so, "-fPIC", "-shared")
    lib = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    lib.qj_ub.restype = C.c_double
    lib.qj_ub.argtypes = [C.c_int, u32, C.c_int, u32, u32]
    lib.qj_bound_check.restype = u32
    lib.qj_bound_check.argtypes = [C.c_int, u32, C.c_int]
    lib.qj_need_mask.restype = C.c_int
    lib.qj_need_mask.argtypes = [C.c_int, u32, C.c_int, C.c_double, C.POINTER(u64)]
    lib.qj_score_check.restype = u32
    lib.qj_score_check.argtypes = [u64, C.c_int, u32, C.c_int, u32, C.POINTER(u64)]
    lib.qj_score.restype = C.c_double
    lib.qj_score.argtypes = [C.c_int, u32, C.c_int, C.c_char_p, u32, C.c_char_p, u32]
    lib.qj_replay.restype = C.c_int
    lib.qj_replay.argtypes = [u64, C.c_int, u32, C.c_int, u32, u32, u32, C.c_double, C.c_int, u32, C.c_int, u32, C.POINTER(u64)]
    lib.qj_replay_all.restype = u32
    yield lib
    d.cleanup()


def _cuts(H, kind):
    """-inf, 0, 0.5, 0.8, 1.0, 1.5, and the bound of lengths (7, 9) at q = 2 in multiset mode with its two f64 neighbours"""
    e = H.qj_ub(kind, 2, 0, 7, 9)
    return (-INF, 0.0, 0.5, 0.8, 1.0, 1.5, math.nextafter(e, 0.0), e, math.nextafter(e, 2.0))


# ---- the symbols ----------------------------------------------------------------------------------------------------------------

def test_qgram_join_symbols_are_exported(L):
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    for name in JOIN_NAMES + CLUSTER_NAMES:
        assert getattr(L, name) is not None
        assert "STRSIM_API int " + name + "(strsim_ctx_t *ctx, int kind, uint32_t q, uint32_t qflags," in hdr


def test_qgram_join_leaves_the_abi_version_and_measure_supported_alone(L):
    assert L.strsim_abi_version() == 0x00010007
    for m in range(-1, 28):
        assert L.strsim_measure_supported(m, 3) == 0
    import strsim_amd
    assert not any("qgram" in name for name in strsim_amd.MEASURE_ID)  # no new measure id


# ---- the bound and the need mask ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,q,set_", MODES)
def test_qgram_join_bound_is_the_maximum_over_every_tuple(H, kind, q, set_):
    # no admissible (I, na, nb) scores above qgram_join_ub at any pair of lengths 0 .. 32, and some tuple attains it
    assert H.qj_bound_check(kind, q, set_) == 0


def test_qgram_join_bound_values(H):
    for kind, q, s in MODES:
        assert H.qj_ub(kind, q, s, 0, 0) == 1.0 and H.qj_ub(kind, q, s, 0, 5) == 0.0 and H.qj_ub(kind, q, s, 32, 0) == 0.0
        for l in range(33):
            assert H.qj_ub(kind, q, s, l, l) == 1.0
        for lq in range(33):
            for lc in range(33):
                assert H.qj_ub(kind, q, s, lq, lc) == H.qj_ub(kind, q, s, lc, lq)
                if lq >= q and lc >= q and (s or kind == 2):
                    assert H.qj_ub(kind, q, s, lq, lc) == 1.0  # set mode and overlap are not pruned by length
    # both shorter than q: equal lengths can be equal strings, unequal ones cannot; one side without a gram is 0.0
    assert H.qj_ub(0, 3, 0, 2, 2) == 1.0 and H.qj_ub(0, 3, 0, 1, 2) == 0.0 and H.qj_ub(0, 3, 1, 2, 5) == 0.0
    # lengths (7, 9) at q = 2: 6 and 8 grams
    assert H.qj_ub(0, 2, 0, 7, 9) == 6.0 / 8.0 and H.qj_ub(1, 2, 0, 7, 9) == 12.0 / 14.0
    assert H.qj_ub(2, 2, 0, 7, 9) == 1.0 and H.qj_ub(3, 2, 0, 7, 9) == 6.0 / math.sqrt(48.0)
    assert H.qj_ub(1, 3, 0, 7, 9) == 10.0 / 12.0 and H.qj_ub(1, 1, 0, 7, 9) == 14.0 / 16.0


@pytest.mark.parametrize("kind,q,set_", MODES)
def test_qgram_join_need_mask_is_the_direct_comparison(H, kind, q, set_):
    w = (C.c_uint64 * 33)()
    for cut in _cuts(H, kind):
        any_bit = H.qj_need_mask(kind, q, set_, cut, w)
        for lq in range(33):
            want = sum(1 << lc for lc in range(33) if H.qj_ub(kind, q, set_, lq, lc) >= cut)
            assert w[lq] == want, (cut, lq)
        assert any_bit == (1 if cut <= 1.0 else 0)


def test_qgram_join_need_mask_at_the_bound_and_its_neighbours(H):
    w = (C.c_uint64 * 33)()
    for kind in (0, 1, 3):  # (overlap's bound at (7, 9) is 1.0: its upper neighbour admits nothing at all)
        e = H.qj_ub(kind, 2, 0, 7, 9)
        assert 0.5 < e < 1.0
        H.qj_need_mask(kind, 2, 0, e, w)
        assert (w[7] >> 9) & 1 and (w[9] >> 7) & 1
        H.qj_need_mask(kind, 2, 0, math.nextafter(e, 2.0), w)
        assert not (w[7] >> 9) & 1 and not (w[9] >> 7) & 1
        H.qj_need_mask(kind, 2, 0, 0.8, w)  # pruned: a strict subset of the lengths
        assert 0 < bin(w[20]).count("1") < 33
    H.qj_need_mask(2, 2, 0, 1.0, w)
    assert all(w[lq] == sum(1 << lc for lc in range(2, 33)) for lq in range(2, 33))  # overlap: every length with a gram
    H.qj_need_mask(0, 2, 1, 1.0, w)
    assert all(w[lq] == sum(1 << lc for lc in range(2, 33)) for lq in range(2, 33))  # set mode likewise


# ---- the scoring call -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alphabet", range(5))
@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("set_", [0, 1])
def test_qgram_join_scoring_call_equals_brute_force(H, alphabet, q, set_):
    # every pair of lengths 0 .. 32 over "a", "ab", "abcdefgh", all 128 ASCII bytes and {NUL, a}; four kinds; both plane forms
    stats = (C.c_uint64 * 3)()
    assert H.qj_score_check(3, alphabet, q, set_, 3, stats) == 0
    assert stats[0] >= 33 * 33 * 3 * 4
    if alphabet <= 2:
        assert stats[1] * 2 == stats[0]  # lower-case letters: every pair in the 5-plane form too
    if alphabet == 4:
        assert stats[1] < stats[0] // 4  # NUL beside a letter: bits 5 and 6 disagree, seven planes


def test_qgram_join_scoring_call_known_answers(H):
    for a, b, kind, q, multiset, want in R.KNOWN:
        got = H.qj_score(KINDS.index(kind), q, 0 if multiset else 1, a.encode(), len(a), b.encode(), len(b))
        assert got == want, (a, b, kind, q, multiset)
    # NULs are characters: "a\0" against "a\0\0" at q = 2 shares the gram (a, NUL)
    assert H.qj_score(1, 2, 0, b"a\0", 2, b"a\0\0", 3) == 2.0 / 3.0 and H.qj_score(0, 2, 1, b"a\0", 2, b"a\0\0", 3) == 0.5
    assert H.qj_score(0, 3, 0, b"a\0", 2, b"a\0", 2) == 1.0 and H.qj_score(0, 3, 0, b"a\0", 2, b"a", 1) == 0.0


# ---- the rules of the sweep -----------------------------------------------------------------------------------------------------

def test_qgram_join_sweeps_replay_against_brute_force(H):
    # four kinds, q 1 .. 3, both modes, every cutoff of the list, with and without upper, 1 .. 3 splits, hit-map groups of 1, 2 and 4
    assert H.qj_replay_all() == 0


@pytest.mark.parametrize("kind", range(4))
@pytest.mark.parametrize("upper", [0, 1])
def test_qgram_join_sweep_finds_every_hit_once_inside_its_segment(H, kind, upper):
    stats = (C.c_uint64 * 3)()
    for cut in _cuts(H, kind):
        for seed, q, set_, nq, nc, maxlen, splits, shift in ((1, 2, 0, 64, 150, 32, 1, 0), (2, 3, 1, 64, 150, 32, 3, 1), (3, 1, 0, 17, 129, 32, 3, 2),
                                                            (4, 2, 1, 64, 120, 5, 2, 0), (5, 3, 0, 1, 90, 32, 2, 1)):
            for under in (0, 1):
                assert H.qj_replay(seed, kind, q, set_, nq, nc, maxlen, cut, upper, splits, under, shift, stats) == 0, (cut, seed, under)
            if cut <= 0.0 and not upper:
                assert stats[0] == nc and stats[1] == nq * nc  # no cutoff: every candidate is visited, every pair is a hit
            if cut > 1.0:
                assert stats[0] == 0 and stats[1] == 0         # nothing is admissible: no sweep


def test_qgram_join_pruning_skips_lengths_in_multiset_mode_only(H):
    stats = (C.c_uint64 * 3)()
    for kind in range(4):
        assert H.qj_replay(12, kind, 2, 0, 1, 400, 32, 0.8, 0, 2, 0, 0, stats) == 0
        pruned = bin(stats[2]).count("1") < 31 and stats[0] < 400
        assert pruned == (kind != 2), kind  # Jaccard, Dice and cosine skip lengths at 0.8; overlap visits every length with a gram
        assert H.qj_replay(12, kind, 2, 1, 1, 400, 32, 0.8, 0, 2, 0, 0, stats) == 0
        assert bin(stats[2]).count("1") >= 31  # set mode: every length with a gram


def test_qgram_join_harness_stands_alone(tmp_path):
    # the same checks as a program of its own (the form that is run under the sanitizers)
    exe = str(tmp_path / "qgram_join_harness")
    _build(exe, "-DQGRAM_JOIN_HARNESS_MAIN")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 length pairs off their bound, 0 mask bits differ, 0 scores differ, 0 replays failed" in out.stdout


# ---- the reference model --------------------------------------------------------------------------------------------------------

def test_qgram_join_ref_known_answers():
    for a, b, kind, q, multiset, want in R.KNOWN:
        assert qgram_ref.score(kind, a, b, q, multiset) == want
        ip, ix, sc = R.join(kind, [a], [b], want, q, multiset)
        assert ip.tolist() == [0, 1] and ix.tolist() == [0] and sc.tolist() == [want]  # in at its own score
        assert R.join(kind, [a], [b], math.nextafter(want, 2.0), q, multiset)[0].tolist() == [0, 0]  # out at the next double
    # abc / cba: out at any positive cutoff for q = 2, in at every cutoff up to 1.0 for q = 1
    assert R.join("sorensen_dice", ["abc"], ["cba"], 5e-324, 2)[0].tolist() == [0, 0]
    assert R.join("sorensen_dice", ["abc"], ["cba"], 0.0, 2)[0].tolist() == [0, 1]
    assert R.join("sorensen_dice", ["abc"], ["cba"], 1.0, 1)[0].tolist() == [0, 1]


def test_qgram_join_ref_csr_and_upper():
    X = ["night", "nacht", "nigh", "night", "", "n"]
    ip, ix, sc = R.join("sorensen_dice", X, X, 0.5, 2)
    assert ip.tolist() == [0, 3, 4, 7, 10, 11, 12] and ix.tolist() == [0, 2, 3, 1, 0, 2, 3, 0, 2, 3, 4, 5]
    assert sc[1] == 6.0 / 7.0 and sc[0] == 1.0
    ip, ix, sc = R.join("sorensen_dice", X, X, 0.5, 2, True, True)
    assert ip.tolist() == [0, 2, 2, 3, 3, 3, 3] and ix.tolist() == [2, 3, 3]
    assert R.join("jaccard", X, X, None, 3, False)[0].tolist() == [0, 6, 12, 18, 24, 30, 36]
    assert R.join("jaccard", [], X, 0.5)[0].tolist() == [0] and R.join("jaccard", X, [], 0.5)[0].tolist() == [0] * 7


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def _join_call(L, name, kind=1, q=2, qflags=0, q_rows=1, c_rows=1, cutoff=-INF, flags=0, capacity=4, null=()):
    qo = (C.c_uint32 * 2)(0, 1)
    qv = (C.c_uint8 * 1)(97)
    indptr = (C.c_uint64 * 4)()
    index = (C.c_uint32 * 4)()
    score = (C.c_double * 4)()
    nnz = C.c_uint64(77)
    arg = lambda key, obj: None if key in null else C.addressof(obj)
    f = getattr(L, name)
    return f(None, kind, q, qflags, arg("q_off", qo), arg("q_val", qv), q_rows, arg("c_off", qo), arg("c_val", qv), c_rows, cutoff, flags, capacity,
             arg("indptr", indptr), arg("index", index), arg("score", score), C.cast(arg("nnz", nnz), C.POINTER(C.c_uint64)))


UNKNOWN_KIND = "unknown kind %d (STRSIM_QGRAM_JACCARD, _SORENSEN_DICE, _OVERLAP or _COSINE: 0..3)"
QGRAM_ERRORS = [
    ("kind4", dict(kind=4), UNKNOWN_KIND % 4),
    ("kind-1", dict(kind=-1), UNKNOWN_KIND % -1),
    ("q0", dict(q=0), "q=0 is outside 1..3"),
    ("q4", dict(q=4), "q=4 is outside 1..3"),
    ("qflags2", dict(qflags=2), "unknown flag bits 0x2 (STRSIM_QGRAM_SET is the only flag)"),
    ("qflags3", dict(qflags=3), "unknown flag bits 0x2 (STRSIM_QGRAM_SET is the only flag)"),
    ("kind_before_q", dict(kind=9, q=0), UNKNOWN_KIND % 9),
    ("q_before_qflags", dict(q=7, qflags=4), "q=7 is outside 1..3"),
]
JOIN_ERRORS = QGRAM_ERRORS + [
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
    ("qflags_before_nan", dict(qflags=8, cutoff=float("nan")), "unknown flag bits 0x8 (STRSIM_QGRAM_SET is the only flag)"),
    ("nan_before_flags", dict(cutoff=float("nan"), flags=8), "min_score is NaN"),
    ("flags_before_rows", dict(flags=2, q_rows=2 ** 32), "unknown flags 0x2 (STRSIM_JOIN_UPPER = 1)"),
    ("rows_before_buffers", dict(q_rows=2 ** 32, null=("q_off", "nnz")), "4294967296 queries (at most 2^32 - 1)"),
    ("buffers_before_nnz", dict(null=("c_val", "nnz")), "NULL candidate buffer"),
    ("nnz_before_indptr", dict(null=("nnz", "indptr")), "out_nnz is NULL"),
    ("indptr_before_outputs", dict(null=("indptr", "index")), "out_indptr is NULL"),
]


@pytest.mark.parametrize("name", JOIN_NAMES)
@pytest.mark.parametrize("case,kw,msg", JOIN_ERRORS)
def test_qgram_join_argument_errors_need_no_device(L, name, case, kw, msg):
    assert _join_call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": " + msg


@pytest.mark.parametrize("name", JOIN_NAMES)
@pytest.mark.parametrize("kw", [dict(), dict(kind=0, q=1), dict(kind=3, q=3, qflags=1), dict(cutoff=0.5), dict(cutoff=1.5), dict(flags=1),
                                dict(capacity=0, null=("index", "score")), dict(q_rows=0, null=("q_off", "q_val")),
                                dict(c_rows=0, null=("c_off", "c_val"))])
def test_qgram_join_null_context_is_checked_last(L, name, kw):
    assert _join_call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": ctx is NULL"


def _cluster_call(L, name, kind=1, q=2, qflags=0, rows=1, min_score=0.5, null=()):
    off = (C.c_uint32 * 2)(0, 1)
    val = (C.c_uint8 * 1)(97)
    root = (C.c_uint32 * 4)()
    cluster = (C.c_uint32 * 4)()
    count, nnz = C.c_uint64(77), C.c_uint64(78)
    arg = lambda key, obj: None if key in null else C.addressof(obj)
    f = getattr(L, name)
    return f(None, kind, q, qflags, arg("off", off), arg("val", val), rows, min_score, arg("root", root), arg("cluster", cluster),
             C.cast(arg("count", count), C.POINTER(C.c_uint64)), C.cast(arg("nnz", nnz), C.POINTER(C.c_uint64)))


CLUSTER_ERRORS = QGRAM_ERRORS + [
    ("nan", dict(min_score=float("nan")), "min_score is NaN"),
    ("too_many_rows", dict(rows=2 ** 32 - 1), "4294967295 rows (at most 2^32 - 2)"),
    ("null_offsets", dict(null=("off",)), "NULL column buffer"),
    ("null_values", dict(null=("val",)), "NULL column buffer"),
    ("null_root", dict(null=("root",)), "out_root is NULL"),
    ("null_count", dict(null=("count",)), "out_count is NULL"),
    ("qflags_before_nan", dict(qflags=2, min_score=float("nan")), "unknown flag bits 0x2 (STRSIM_QGRAM_SET is the only flag)"),
    ("nan_before_rows", dict(min_score=float("nan"), rows=2 ** 32), "min_score is NaN"),
    ("rows_before_buffers", dict(rows=2 ** 32, null=("off",)), "4294967296 rows (at most 2^32 - 2)"),
    ("buffers_before_root", dict(null=("val", "root")), "NULL column buffer"),
    ("root_before_count", dict(null=("root", "count")), "out_root is NULL"),
]


@pytest.mark.parametrize("name", CLUSTER_NAMES)
@pytest.mark.parametrize("case,kw,msg", CLUSTER_ERRORS)
def test_qgram_cluster_argument_errors_need_no_device(L, name, case, kw, msg):
    assert _cluster_call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": " + msg


@pytest.mark.parametrize("name", CLUSTER_NAMES)
@pytest.mark.parametrize("kw", [dict(), dict(kind=0, q=3, qflags=1), dict(min_score=1.5), dict(null=("cluster", "nnz")),
                                dict(rows=0, null=("off", "val", "root"))])
def test_qgram_cluster_null_context_is_checked_last(L, name, kw):
    assert _cluster_call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": ctx is NULL"


def test_join_and_match_join_keep_their_own_words(L):
    # the entry points that share the checks still word their first refusal themselves, before the NaN
    def call(name, measure, cutoff):
        qo, qv, nnz = (C.c_uint32 * 2)(0, 1), (C.c_uint8 * 1)(97), C.c_uint64(0)
        indptr, index, score = (C.c_uint64 * 4)(), (C.c_uint32 * 4)(), (C.c_double * 4)()
        return getattr(L, name)(None, measure, C.addressof(qo), C.addressof(qv), 1, C.addressof(qo), C.addressof(qv), 1, cutoff, 0, 4,
                                C.addressof(indptr), C.addressof(index), C.addressof(score), C.byref(nnz))
    assert call("strsim_match_join_device", 9, float("nan")) == ERR_ARG
    assert L.strsim_last_error_message().decode() == "strsim_match_join_device: measure 9 is not a measure of match_join (the reference measures 0 .. 4)"
    assert call("strsim_join_host", 8, float("nan")) == ERR_ARG
    assert L.strsim_last_error_message().decode() == "strsim_join_host: score_cutoff is NaN"
    assert call("strsim_join_host", 8, 0.5) == ERR_ARG and L.strsim_last_error_message().decode() == "strsim_join_host: ctx is NULL"


# ---- the Python surfaces --------------------------------------------------------------------------------------------------------

def _decode(off, val):
    raw = bytes(val)
    return [raw[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


class _StubContext:
    """strsim_amd.qgram_join / qgram_cluster above the Context's methods, the device replaced by the reference"""
    def __init__(self):
        self.calls = []

    def qgram_join(self, kind, qo, qv, co, cv, min_score=None, upper=False, q=2, multiset=True):
        Q, Cs = _decode(qo, qv), _decode(co, cv)
        self.calls.append((kind, Q, Cs, min_score, upper, q, multiset))
        return R.join(kind, Q, Cs, min_score, q, multiset, upper)

    def qgram_cluster(self, kind, o, v, min_score, q=2, multiset=True):
        import cluster_ref
        X = _decode(o, v)
        self.calls.append((kind, X, min_score, q, multiset))
        return cluster_ref.cluster(None, X, min_score, found=R.join(kind, X, X, min_score, q, multiset, True))[:3]

    def match_join(self, *a, **k):
        raise AssertionError("qgram_join goes through Context.qgram_join")

    join = cluster = match_join

    def default_process_host(self, off, val):
        raise AssertionError("no processor was asked for")


def test_qgram_join_python_surface_errors():
    import strsim_amd
    from strsim_amd.context import Context
    for name in ("qgram_join", "qgram_dedupe_pairs", "qgram_cluster"):
        assert name in strsim_amd.__all__
    assert callable(Context.qgram_join) and callable(Context.qgram_cluster)
    stub = _StubContext()
    for f in (lambda **k: strsim_amd.qgram_join(k.pop("kind", "jaccard"), ["a"], ["b"], 0.5, ctx=stub, **k),
              lambda **k: strsim_amd.qgram_dedupe_pairs(k.pop("kind", "jaccard"), ["a"], 0.5, ctx=stub, **k),
              lambda **k: strsim_amd.qgram_cluster(k.pop("kind", "jaccard"), ["a"], 0.5, ctx=stub, **k)):
        for bad in ("dice", "levenshtein", 1, None):
            with pytest.raises(ValueError, match=r"unknown q-gram kind .*\(one of \('jaccard', 'sorensen_dice', 'overlap', 'cosine'\)\)"):
                f(kind=bad)
        for bad in (0, 4, 2.0, True, None):
            with pytest.raises(ValueError, match=r"q=.* is outside 1 \.\. 3"):
                f(q=bad)
        with pytest.raises(ValueError, match="unknown processor 'lower'"):
            f(processor="lower")
    with pytest.raises(ValueError, match="min_score=None would put every row in one cluster"):
        strsim_amd.qgram_cluster("jaccard", ["a"], None, ctx=stub)
    assert stub.calls == []
    ctx = Context.__new__(Context)
    ctx._h = None
    with pytest.raises(ValueError, match="unknown q-gram kind 'ratio'"):
        ctx.qgram_join("ratio", *strsim_amd.pack_strings(["a"]), *strsim_amd.pack_strings(["a"]), 0.5)
    with pytest.raises(ValueError, match=r"q=5 is outside 1 \.\. 3"):
        ctx.qgram_cluster("jaccard", *strsim_amd.pack_strings(["a"]), 0.5, q=5)


def test_qgram_join_null_handling_and_index_mapping_with_a_stubbed_context():
    import strsim_amd
    Q = ["night", None, "abc", ""]
    Cs = [None, "nacht", "abd", None, "night", ""]
    stub = _StubContext()
    indptr, index, score = strsim_amd.qgram_join("sorensen_dice", Q, Cs, 0.25, ctx=stub)
    assert stub.calls == [("sorensen_dice", ["night", "", "abc", ""], ["nacht", "abd", "night", ""], 0.25, False, 2, True)]
    assert indptr.dtype == np.int64 and index.dtype == np.int64 and score.dtype == np.float64
    assert indptr.tolist() == [0, 2, 2, 3, 4] and index.tolist() == [1, 4, 2, 5] and score.tolist() == [0.25, 1.0, 0.5, 1.0]
    indptr, index, score = strsim_amd.qgram_join("jaccard", Q, Cs, None, q=3, multiset=False, ctx=stub)
    assert stub.calls[-1] == ("jaccard", ["night", "", "abc", ""], ["nacht", "abd", "night", ""], None, False, 3, False)
    assert indptr.tolist() == [0, 4, 4, 8, 12] and index.tolist() == [1, 2, 4, 5] * 3
    assert strsim_amd.qgram_join("cosine", [], ["a"], 0.5, ctx=stub)[0].tolist() == [0]
    assert strsim_amd.qgram_join("cosine", ["a", None], [], 0.5, ctx=stub)[0].tolist() == [0, 0, 0]


def test_qgram_dedupe_pairs_and_cluster_with_a_stubbed_context():
    import strsim_amd
    col = ["night", "nacht", None, "night", "nigh", "nacht", None, ""]
    stub = _StubContext()
    i, j, s = strsim_amd.qgram_dedupe_pairs("sorensen_dice", col, 0.8, ctx=stub)
    assert stub.calls == [("sorensen_dice", [c or "" for c in col], [c or "" for c in col], 0.8, True, 2, True)]
    assert list(zip(i.tolist(), j.tolist())) == [(0, 3), (0, 4), (1, 5), (3, 4)] and s.tolist() == [1.0, 6.0 / 7.0, 1.0, 6.0 / 7.0]
    root, label, count = strsim_amd.qgram_cluster("sorensen_dice", col, 0.8, q=2, ctx=stub)
    assert stub.calls[-1] == ("sorensen_dice", [c for c in col if c is not None], 0.8, 2, True)  # the nulls are dropped, never kept as ""
    assert root.tolist() == [0, 1, -1, 0, 0, 1, -1, 7] and label.tolist() == [0, 1, -1, 0, 0, 1, -1, 2] and count == 3


class _FakeLib:
    """strsim_qgram_join_host as Context.qgram_join calls it: the capacity protocol over a fixed result"""
    def __init__(self, result):
        self.result = result
        self.calls = []

    def strsim_qgram_join_host(self, h, kind, q, qflags, qo, qv, nq, co, cv, nc, cut, flags, capacity, indptr, index, score, nnz):
        ip, ix, sc = self.result
        self.calls.append((capacity, index is None, flags, cut, kind, q, qflags))
        C.memmove(indptr, ip.ctypes.data, ip.nbytes)
        C.cast(nnz, C.POINTER(C.c_uint64))[0] = ix.size
        if ix.size <= capacity and ix.size:
            C.memmove(index, ix.ctypes.data, ix.nbytes)
            C.memmove(score, sc.ctypes.data, sc.nbytes)
        return 0


def test_context_qgram_join_retries_once_with_the_exact_size(monkeypatch):
    import strsim_amd
    from strsim_amd import context
    Q, Cs = ["ab", "abc", "b"], ["ab", "abc", "abd", "b"]
    exp = R.join("cosine", Q, Cs, 0.3, 1)
    fake = _FakeLib(exp)
    monkeypatch.setattr(context, "lib", lambda: fake)
    ctx = context.Context.__new__(context.Context)
    ctx._h = None
    cols = (*strsim_amd.pack_strings(Q), *strsim_amd.pack_strings(Cs))
    n = exp[1].size
    assert n > 3
    assert R.same(ctx.qgram_join("cosine", *cols, 0.3, q=1, capacity=3), exp) and [c[0] for c in fake.calls] == [3, n]
    fake.calls.clear()
    assert R.same(ctx.qgram_join("cosine", *cols, 0.3, q=1), exp) and [c[0] for c in fake.calls] == [4 * 3 + 1024]  # the guess holds
    fake.calls.clear()
    assert R.same(ctx.qgram_join("cosine", *cols, 0.3, True, 3, False, capacity=n), exp) and fake.calls == [(n, False, 1, 0.3, 3, 3, 1)]
    fake.calls.clear()
    assert np.array_equal(ctx.qgram_join("overlap", *cols, None, count_only=True), exp[0]) and fake.calls == [(0, True, 0, -INF, 2, 2, 0)]


# ---- the frames of the GPU tests --------------------------------------------------------------------------------------------------

def test_qgram_join_gpu_frames_are_not_vacuous():
    # every parity frame of tests/test_qgram_join_gpu.py at its cutoffs: 0 < nnz < nq * nc on the reference side
    import qgram_join_frames as F
    for kind in KINDS:
        for q, multiset in F.MODES:
            assert F.not_vacuous(F.known_matrix(kind, q, multiset), F.KNOWN_CUT), (kind, q, multiset)
            B = F.boundary_matrix(kind, q, multiset)
            assert F.not_vacuous(B, F.BOUNDARY_CUT) and F.not_vacuous(B, 1.0) and F.not_vacuous(B, F.BOUNDARY_CUT, True), (kind, q, multiset)
    for kind, q, multiset in (("sorensen_dice", 2, True), ("jaccard", 3, False)):
        M = F.near_matrix(kind, q, multiset)
        for nq in F.GEOMETRY_NQ:
            for nc in F.GEOMETRY_NC:
                for upper in (False, True):
                    assert F.not_vacuous(M[:nq, :nc], F.GEOMETRY_CUT, upper), (kind, nq, nc, upper)
    Q, Cs = F.boundary(2)
    assert {len(s.encode()) for s in Q} >= {0, 1, 2, 3, 31, 32, 33} and {len(s.encode()) for s in Cs} >= {0, 1, 2, 3, 31, 32, 33}
    assert any(not s.isascii() and len(s.encode()) <= 32 for s in Q) and any(not s.isascii() and len(s.encode()) <= 32 for s in Cs)


# ---- the plugin's surfaces ------------------------------------------------------------------------------------------------------

def test_qgram_join_plugin_symbols_and_polars_wrapper_source(L):
    plug = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    for kind in KINDS:
        for family in ("qgram_join_", "qgram_cluster_"):
            assert getattr(L, "_polars_plugin_" + family + kind) is not None and getattr(L, "_polars_plugin_field_" + family + kind) is not None
            assert "POLARS_PLUGIN_DECLARE(%s%s)" % (family, kind) in plug
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    compile(src, "polars_strsim/__init__.py", "exec")
    assert '__all__ += ["qgram_join", "qgram_cluster"]' in src
    assert ('def qgram_join(expr: IntoExpr, candidates: IntoExpr, kind: str = "sorensen_dice", q: int = 2, multiset: bool = True,\n'
            '               min_score: float | None = None) -> pl.Expr:') in src
    assert ('def qgram_cluster(expr: IntoExpr, kind: str = "sorensen_dice", q: int = 2, multiset: bool = True, min_score: float | None = None)'
            ' -> pl.Expr:') in src
    body = src[src.index("def qgram_join("):]
    for word in ("is_elementwise=False", '"qgram_join_" + kind', '"qgram_cluster_" + kind', "pl.lit(min_score, dtype=pl.Float64)",
                 "pl.lit(q, dtype=pl.UInt32)", "min_score is required"):
        assert word in body or word in src[src.index("def _qgram_mode("):], word


@pytest.mark.parametrize("kind", KINDS)
def test_qgram_join_plugin_fields(kind):
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    want = pa.large_list(pa.field("item", pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])))
    assert arrow_host.field_plugin("qgram_join_" + kind, ("queries", "cands", "q", "set", "min_score")) == ("queries", want)
    assert arrow_host.field_plugin("qgram_cluster_" + kind, ("name", "q", "set", "min_score")) == ("name", pa.uint32())


def test_qgram_join_plugin_argument_errors_need_no_device():
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host as H
    u32 = lambda v: pa.array([v], type=pa.uint32())
    LIST = pa.large_list(pa.field("item", pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])))
    for extra, words in (([], "qgram_join: expected 2 input series .*got 2"), ([u32(0), u32(0)], "q=0 is outside 1..3"),
                         ([u32(2), u32(2)], "the set flag must be 0 or 1, got 2"),
                         ([u32(2), u32(0), pa.array([float("nan")], type=pa.float64())], "score_cutoff must not be NaN")):
        with pytest.raises(H.PluginError, match=words):
            H.call_plugin("qgram_join_jaccard", ["abc"], ["abd"], out_type=LIST, extra=extra)
    for b, extra, words in ((u32(2), [], "qgram_cluster: expected 4 input series .*got 2"), (u32(5), [u32(0), pa.array([0.5])], "q=5 is outside 1..3"),
                            (u32(2), [u32(0), pa.array([None], type=pa.float64())], "min_score must not be null")):
        with pytest.raises(H.PluginError, match=words):
            H.call_plugin("qgram_cluster_cosine", ["abc", "abd"], b, out_type=pa.uint32(), extra=extra)
