"""distance_join / distance_cluster (the join by integer edit distance) without a GPU: the exported symbols, every argument error of
the four entry points before any device and the order of the checks, the three facts of the Damerau-Levenshtein filter and the
sweep's decision over every pair of short strings, the need mask, a wave's count and fill sweeps replayed (strsim_distance_join.h
compiled by g++), the reference model against hand-written answers, the Python surfaces with the context stubbed, the plugin's
surfaces, and the frames of the GPU tests shown not to be vacuous."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import damerau_ref
import distance_join_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "distance_join_harness.cpp")
ERR_ARG = 2
UNBOUNDED = 0xFFFFFFFF
JOIN_NAMES = ("strsim_distance_join_device", "strsim_distance_join_host")
CLUSTER_NAMES = ("strsim_distance_cluster_device", "strsim_distance_cluster_host")
MEASURES = R.MEASURES


@pytest.fixture(scope="module")
def L():
    import strsim_amd
    return strsim_amd.lib()  # (a library without strsim_distance_join_device fails here: nothing is skipped)


def _build(out, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", CSRC, *flags, "-o", out, HARNESS])


@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="distance_join_harness_")
    so = os.path.join(d.name, "libdistance_join_harness.so")
    _build(so, "-fPIC", "-shared")
    lib = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    lib.dj_facts_check.restype = u32
    lib.dj_facts_check.argtypes = [u32, u32, C.POINTER(u64)]
    lib.dj_need_mask.restype = None
    lib.dj_need_mask.argtypes = [u32, C.POINTER(u64)]
    lib.dj_need_check.restype = u32
    lib.dj_need_check.argtypes = [u32]
    lib.dj_cutoff.restype = C.c_double
    lib.dj_cutoff.argtypes = [u32]
    lib.dj_distance.restype = u32
    lib.dj_distance.argtypes = [C.c_int, u32, C.c_char_p, u32, C.c_char_p, u32]
    lib.dj_replay.restype = C.c_int
    lib.dj_replay.argtypes = [u64, C.c_int, u32, u32, u32, u32, C.c_int, u32, C.c_int, u32, C.POINTER(u64)]
    lib.dj_replay_all.restype = u32
    yield lib
    d.cleanup()


# ---- the symbols ----------------------------------------------------------------------------------------------------------------

def test_distance_join_symbols_are_exported(L):
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    for name in JOIN_NAMES + CLUSTER_NAMES:
        assert getattr(L, name) is not None
        assert "STRSIM_API int " + name + "(strsim_ctx_t *ctx, int kind," in hdr
    assert "enum { STRSIM_EDIT_LEVENSHTEIN = 0, STRSIM_EDIT_OSA = 1, STRSIM_EDIT_DAMERAU = 2 };" in hdr


def test_distance_join_leaves_the_abi_version_and_measure_supported_alone(L):
    assert L.strsim_abi_version() == 0x00010007
    for m in range(-1, 28):
        assert L.strsim_measure_supported(m, 3) == 0
    import strsim_amd
    assert not any("damerau" in name or "distance_join" in name for name in strsim_amd.MEASURE_ID)  # no new measure id
    assert strsim_amd.DISTANCE_JOIN_MEASURES == MEASURES


# ---- the filter, the need mask and the sweep (the host harness) -----------------------------------------------------------------

@pytest.mark.parametrize("alphabet,maxlen,strings", [(3, 5, 364), (2, 7, 255)])
def test_distance_join_three_facts_and_the_decision_over_every_pair(H, alphabet, maxlen, strings):
    # every ordered pair of strings over "abc" up to 5 bytes and over "ab" up to 7; k = 0 .. 4 and unbounded
    stats = (C.c_uint64 * 7)()
    assert H.dj_facts_check(alphabet, maxlen, stats) == 0
    assert stats[0] == strings * strings and stats[1] == 0 and stats[4] == 0 and stats[5] == 0
    assert stats[3] > 0 and stats[6] > 0  # undecided pairs, and the cell DP ran
    assert (stats[2] > 0) == (alphabet == 3)  # pairs with dl < osa: a swap across a third byte


def test_distance_join_need_mask_is_the_length_window(H):
    w = (C.c_uint64 * 33)()
    for k in (0, 1, 2, 3, 4, 31, 32, 33, UNBOUNDED - 1, UNBOUNDED):
        assert H.dj_need_check(k) == 0
        H.dj_need_mask(k, w)
        for lq in range(33):
            assert w[lq] == sum(1 << lc for lc in range(33) if abs(lq - lc) <= k), (k, lq)
    H.dj_need_mask(2, w)
    assert sum(bin(w[lq] & ~1).count("1") for lq in range(1, 33)) == 154  # of the 1 024 pairs of lengths 1 .. 32
    assert H.dj_cutoff(0) == 0.0 and H.dj_cutoff(7) == -7.0 and H.dj_cutoff(UNBOUNDED - 1) == -4294967294.0 and H.dj_cutoff(UNBOUNDED) == -np.inf


def test_distance_join_scoring_calls_known_answers(H):
    for a, b, lev, osa, dl in R.KNOWN:
        if not (a.isascii() and b.isascii()):
            continue
        for k in (0, 1, 2, 3, UNBOUNDED):
            assert H.dj_distance(0, k, a.encode(), len(a), b.encode(), len(b)) == lev
            assert H.dj_distance(1, k, a.encode(), len(a), b.encode(), len(b)) == osa
            got = H.dj_distance(2, k, a.encode(), len(a), b.encode(), len(b))
            assert (got <= k) == (dl <= k) and (got == dl or dl > k), (a, b, k)
    # ("ca", "abc"): osa 3 is undecided at k = 2 and the cell DP finds 2; at k = 1 it is decided (3 > 2 k) and stays 3
    assert H.dj_distance(2, 2, b"ca", 2, b"abc", 3) == 2 and H.dj_distance(2, 1, b"ca", 2, b"abc", 3) == 3


def test_distance_join_sweeps_replay_against_brute_force(H):
    # three kinds, k = 0 .. 4 and unbounded, with and without upper, 1 .. 3 splits, hit-map groups of 1, 2 and 4, guard words
    assert H.dj_replay_all() == 0


@pytest.mark.parametrize("kind", range(3))
@pytest.mark.parametrize("upper", [0, 1])
def test_distance_join_sweep_finds_every_hit_once_inside_its_segment(H, kind, upper):
    stats = (C.c_uint64 * 3)()
    for k in (0, 1, 2, 3, 4, UNBOUNDED):
        for seed, nq, nc, maxlen, splits, shift in ((1, 64, 150, 32, 1, 0), (2, 64, 150, 32, 3, 1), (3, 17, 129, 32, 3, 2), (4, 64, 120, 5, 2, 0),
                                                    (5, 1, 90, 32, 2, 1)):
            for under in (0, 1):
                assert H.dj_replay(seed, kind, k, nq, nc, maxlen, upper, splits, under, shift, stats) == 0, (k, seed, under)
            if k == UNBOUNDED and not upper:
                assert stats[0] == nc and stats[1] == nq * nc  # no cutoff: every candidate is visited, every pair is a hit


def test_distance_join_pruning_visits_the_window_only(H):
    stats = (C.c_uint64 * 3)()
    for kind in range(3):
        assert H.dj_replay(12, kind, 2, 1, 400, 32, 0, 2, 0, 0, stats) == 0
        assert 1 <= bin(stats[2]).count("1") <= 5 and stats[0] < 400  # one query at k = 2: at most five lengths
        assert H.dj_replay(12, kind, UNBOUNDED, 1, 400, 32, 0, 2, 0, 0, stats) == 0
        assert bin(stats[2]).count("1") == 33 and stats[0] == 400


def test_distance_join_harness_stands_alone(tmp_path):
    # the same checks as a program of its own (the form that is run under the sanitizers)
    exe = str(tmp_path / "distance_join_harness")
    _build(exe, "-DDISTANCE_JOIN_HARNESS_MAIN")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "197521 ordered pairs, 0 fact violations, 0 decisions differ, 0 cores differ" in out.stdout
    assert "0 mask bits differ, 0 replays failed" in out.stdout


# ---- the reference model --------------------------------------------------------------------------------------------------------

def test_distance_join_ref_known_answers():
    for a, b, lev, osa, dl in R.KNOWN:
        for x, y in ((a, b), (b, a)):
            assert int(R.pairs("levenshtein", [x], [y])[0]) == lev and int(R.pairs("osa", [x], [y])[0]) == osa
            assert damerau_ref.distance(x, y) == dl
        for measure, d in zip(MEASURES, (lev, osa, dl)):
            ip, ix, ds = R.join(measure, [a], [b], d)
            assert ip.tolist() == [0, 1] and ix.tolist() == [0] and ds.tolist() == [d]  # in at its own distance
            if d:
                assert R.join(measure, [a], [b], d - 1)[0].tolist() == [0, 0]           # out one below
    assert R.KNOWN[0][:2] == ("ca", "abc") and R.KNOWN[0][2:] == (3, 3, 2) and R.KNOWN[1][:2] == ("ca", "ac") and R.KNOWN[1][2:] == (2, 1, 1)
    # the vectorised DPs side by side equal one pair at a time, and the C form of the Damerau DP equals the Python form
    A = ["kitten", "", "abcdef", "ca", "a cat", "x"]
    B = ["sitting", "abc", "badcfe", "abc", "an abct", ""]
    for measure in ("levenshtein", "osa"):
        assert R.pairs(measure, A, B).tolist() == [int(R.pairs(measure, [a], [b])[0]) for a, b in zip(A, B)]
    assert R.pairs("levenshtein", A, B).tolist() == [3, 3, 4, 3, 4, 1] and R.pairs("osa", A, B).tolist() == [3, 3, 3, 3, 4, 1]
    assert [R._cref().distance(a, b) for a, b in zip(A, B)] == [damerau_ref.distance(a, b) for a, b in zip(A, B)] == [3, 3, 3, 2, 3, 1]


def test_distance_join_ref_csr_and_upper():
    X = ["night", "nacht", "nigh", "night", "", "n"]
    ip, ix, ds = R.join("levenshtein", X, X, 1)
    assert ip.tolist() == [0, 3, 4, 7, 10, 12, 14] and ix.tolist() == [0, 2, 3, 1, 0, 2, 3, 0, 2, 3, 4, 5, 4, 5]
    assert ds.tolist() == [0, 1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0] and ds.dtype == np.uint32 and ix.dtype == np.uint32 and ip.dtype == np.uint64
    ip, ix, ds = R.join("osa", X, X, 1, True)
    assert ip.tolist() == [0, 2, 2, 3, 3, 4, 4] and ix.tolist() == [2, 3, 3, 5]
    assert R.join("damerau_levenshtein", X, X, None)[0].tolist() == [0, 6, 12, 18, 24, 30, 36]
    assert R.join("osa", X, X, 0)[1].tolist() == [0, 3, 1, 2, 0, 3, 4, 5]
    assert R.join("osa", [], X, 1)[0].tolist() == [0] and R.join("osa", X, [], 1)[0].tolist() == [0] * 7
    M = R.matrix("damerau_levenshtein", ["ca", "ac"], ["abc", "ca"])
    assert M.tolist() == [[2, 0], [1, 1]]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def _join_call(L, name, kind=0, q_rows=1, c_rows=1, k=2, flags=0, capacity=4, null=()):
    qo = (C.c_uint32 * 2)(0, 1)
    qv = (C.c_uint8 * 1)(97)
    indptr = (C.c_uint64 * 4)()
    index = (C.c_uint32 * 4)()
    dist = (C.c_uint32 * 4)()
    nnz = C.c_uint64(77)
    arg = lambda key, obj: None if key in null else C.addressof(obj)
    f = getattr(L, name)
    return f(None, kind, arg("q_off", qo), arg("q_val", qv), q_rows, arg("c_off", qo), arg("c_val", qv), c_rows, k, flags, capacity,
             arg("indptr", indptr), arg("index", index), arg("dist", dist), C.cast(arg("nnz", nnz), C.POINTER(C.c_uint64)))


UNKNOWN_KIND = "unknown kind %d (STRSIM_EDIT_LEVENSHTEIN, _OSA or _DAMERAU: 0..2)"
KIND_ERRORS = [
    ("kind3", dict(kind=3), UNKNOWN_KIND % 3),
    ("kind-1", dict(kind=-1), UNKNOWN_KIND % -1),
    ("kind17", dict(kind=17), UNKNOWN_KIND % 17),  # (STRSIM_OSA's measure id is no kind)
]
JOIN_ERRORS = KIND_ERRORS + [
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
    ("null_distance", dict(null=("dist",)), "capacity=4 with a NULL output buffer"),
    ("kind_before_flags", dict(kind=5, flags=8), UNKNOWN_KIND % 5),
    ("flags_before_rows", dict(flags=2, q_rows=2 ** 32), "unknown flags 0x2 (STRSIM_JOIN_UPPER = 1)"),
    ("rows_before_buffers", dict(q_rows=2 ** 32, null=("q_off", "nnz")), "4294967296 queries (at most 2^32 - 1)"),
    ("buffers_before_nnz", dict(null=("c_val", "nnz")), "NULL candidate buffer"),
    ("nnz_before_indptr", dict(null=("nnz", "indptr")), "out_nnz is NULL"),
    ("indptr_before_outputs", dict(null=("indptr", "index")), "out_indptr is NULL"),
]


@pytest.mark.parametrize("name", JOIN_NAMES)
@pytest.mark.parametrize("case,kw,msg", JOIN_ERRORS)
def test_distance_join_argument_errors_need_no_device(L, name, case, kw, msg):
    assert _join_call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": " + msg


@pytest.mark.parametrize("name", JOIN_NAMES)
@pytest.mark.parametrize("kw", [dict(), dict(kind=1, k=0), dict(kind=2, k=UNBOUNDED), dict(flags=1), dict(capacity=0, null=("index", "dist")),
                                dict(q_rows=0, null=("q_off", "q_val")), dict(c_rows=0, null=("c_off", "c_val"))])
def test_distance_join_null_context_is_checked_last(L, name, kw):
    assert _join_call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": ctx is NULL"


def _cluster_call(L, name, kind=0, rows=1, k=2, null=()):
    off = (C.c_uint32 * 2)(0, 1)
    val = (C.c_uint8 * 1)(97)
    root = (C.c_uint32 * 4)()
    cluster = (C.c_uint32 * 4)()
    count, nnz = C.c_uint64(77), C.c_uint64(78)
    arg = lambda key, obj: None if key in null else C.addressof(obj)
    f = getattr(L, name)
    return f(None, kind, arg("off", off), arg("val", val), rows, k, arg("root", root), arg("cluster", cluster),
             C.cast(arg("count", count), C.POINTER(C.c_uint64)), C.cast(arg("nnz", nnz), C.POINTER(C.c_uint64)))


CLUSTER_ERRORS = KIND_ERRORS + [
    ("too_many_rows", dict(rows=2 ** 32 - 1), "4294967295 rows (at most 2^32 - 2)"),
    ("null_offsets", dict(null=("off",)), "NULL column buffer"),
    ("null_values", dict(null=("val",)), "NULL column buffer"),
    ("null_root", dict(null=("root",)), "out_root is NULL"),
    ("null_count", dict(null=("count",)), "out_count is NULL"),
    ("kind_before_rows", dict(kind=3, rows=2 ** 32), UNKNOWN_KIND % 3),
    ("rows_before_buffers", dict(rows=2 ** 32, null=("off",)), "4294967296 rows (at most 2^32 - 2)"),
    ("buffers_before_root", dict(null=("val", "root")), "NULL column buffer"),
    ("root_before_count", dict(null=("root", "count")), "out_root is NULL"),
]


@pytest.mark.parametrize("name", CLUSTER_NAMES)
@pytest.mark.parametrize("case,kw,msg", CLUSTER_ERRORS)
def test_distance_cluster_argument_errors_need_no_device(L, name, case, kw, msg):
    assert _cluster_call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": " + msg


@pytest.mark.parametrize("name", CLUSTER_NAMES)
@pytest.mark.parametrize("kw", [dict(), dict(kind=2, k=UNBOUNDED), dict(kind=1, k=0), dict(null=("cluster", "nnz")),
                                dict(rows=0, null=("off", "val", "root"))])
def test_distance_cluster_null_context_is_checked_last(L, name, kw):
    assert _cluster_call(L, name, **kw) == ERR_ARG
    assert L.strsim_last_error_message().decode() == name + ": ctx is NULL"


# ---- the Python surfaces --------------------------------------------------------------------------------------------------------

def _decode(off, val):
    raw = bytes(val)
    return [raw[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


class _StubContext:
    """strsim_amd.distance_join / distance_cluster above the Context's methods, the device replaced by the reference"""
    def __init__(self):
        self.calls = []

    def distance_join(self, kind, qo, qv, co, cv, max_distance=None, upper=False):
        Q, Cs = _decode(qo, qv), _decode(co, cv)
        self.calls.append((kind, Q, Cs, max_distance, upper))
        return R.join(kind, Q, Cs, max_distance, upper)

    def distance_cluster(self, kind, o, v, max_distance):
        import cluster_ref
        X = _decode(o, v)
        self.calls.append((kind, X, max_distance))
        return cluster_ref.cluster(None, X, max_distance, found=R.join(kind, X, X, max_distance, True))[:3]

    def match_join(self, *a, **k):
        raise AssertionError("distance_join goes through Context.distance_join")

    join = cluster = qgram_join = qgram_cluster = match_join

    def default_process_host(self, off, val):
        raise AssertionError("no processor was asked for")


def test_distance_join_python_surface_errors():
    import strsim_amd
    from strsim_amd.context import Context
    assert strsim_amd.__all__[-4:] == ["distance_join", "distance_dedupe_pairs", "distance_cluster", "DISTANCE_JOIN_MEASURES"]
    assert callable(Context.distance_join) and callable(Context.distance_cluster)
    stub = _StubContext()
    for f in (lambda **k: strsim_amd.distance_join(k.pop("measure", "osa"), ["a"], ["b"], 1, ctx=stub, **k),
              lambda **k: strsim_amd.distance_dedupe_pairs(k.pop("measure", "osa"), ["a"], 1, ctx=stub, **k),
              lambda **k: strsim_amd.distance_cluster(k.pop("measure", "osa"), ["a"], 1, ctx=stub, **k)):
        for bad in ("damerau", "indel", "jaro", 1, None):
            with pytest.raises(ValueError, match=r"unknown edit distance .*\(one of \('levenshtein', 'osa', 'damerau_levenshtein'\)\)"):
                f(measure=bad)
        with pytest.raises(ValueError, match="unknown processor 'lower'"):
            f(processor="lower")
    with pytest.raises(ValueError, match="cluster: max_distance=None would put every row in one cluster"):
        strsim_amd.distance_cluster("osa", ["a"], None, ctx=stub)
    with pytest.raises(ValueError, match=r"cluster: min_score=None would put every row in one cluster; pass a score in \[0, 1\]"):
        strsim_amd.cluster("jaro", ["a"], None, ctx=stub)  # the existing callers keep their sentence
    assert stub.calls == []
    ctx = Context.__new__(Context)
    ctx._h = None
    cols = (*strsim_amd.pack_strings(["a"]), *strsim_amd.pack_strings(["a"]))
    with pytest.raises(ValueError, match="unknown edit distance 'ratio'"):
        ctx.distance_join("ratio", *cols, 1)
    with pytest.raises(ValueError, match="max_distance=-1 is outside"):
        ctx.distance_join("osa", *cols, -1)
    with pytest.raises(ValueError, match="max_distance=4294967296 is outside"):
        ctx.distance_cluster("osa", *cols[:2], 2 ** 32)


def test_distance_join_null_handling_and_index_mapping_with_a_stubbed_context():
    import strsim_amd
    Q = ["night", None, "abc", ""]
    Cs = [None, "nacht", "abd", None, "night", ""]
    stub = _StubContext()
    indptr, index, dist = strsim_amd.distance_join("levenshtein", Q, Cs, 2, ctx=stub)
    assert stub.calls == [("levenshtein", ["night", "", "abc", ""], ["nacht", "abd", "night", ""], 2, False)]
    assert indptr.dtype == np.int64 and index.dtype == np.int64 and dist.dtype == np.uint32
    assert indptr.tolist() == [0, 2, 2, 3, 4] and index.tolist() == [1, 4, 2, 5] and dist.tolist() == [2, 0, 1, 0]
    indptr, index, dist = strsim_amd.distance_join("damerau_levenshtein", Q, Cs, None, ctx=stub)
    assert stub.calls[-1] == ("damerau_levenshtein", ["night", "", "abc", ""], ["nacht", "abd", "night", ""], None, False)
    assert indptr.tolist() == [0, 4, 4, 8, 12] and index.tolist() == [1, 2, 4, 5] * 3 and dist.tolist() == [2, 5, 0, 5, 4, 1, 5, 3, 5, 3, 5, 0]
    # upper keeps the positions: the null candidates stay, as empty strings, and their hits are dropped
    indptr, index, dist = strsim_amd.distance_join("osa", ["ab", None, "ba"], ["ab", None, "ba", "ab"], 1, upper=True, ctx=stub)
    assert stub.calls[-1] == ("osa", ["ab", "", "ba"], ["ab", "", "ba", "ab"], 1, True)
    assert indptr.tolist() == [0, 2, 2, 3] and index.tolist() == [2, 3, 3] and dist.tolist() == [1, 0, 1]
    assert strsim_amd.distance_join("osa", [], ["a"], 1, ctx=stub)[0].tolist() == [0]
    assert strsim_amd.distance_join("osa", ["a", None], [], 1, ctx=stub)[0].tolist() == [0, 0, 0]


def test_distance_dedupe_pairs_and_cluster_with_a_stubbed_context():
    import strsim_amd
    col = ["night", "nacht", None, "night", "nigth", "nacht", None, ""]
    stub = _StubContext()
    i, j, d = strsim_amd.distance_dedupe_pairs("osa", col, 1, ctx=stub)
    assert stub.calls == [("osa", [c or "" for c in col], [c or "" for c in col], 1, True)]
    assert list(zip(i.tolist(), j.tolist())) == [(0, 3), (0, 4), (1, 5), (3, 4)] and d.tolist() == [0, 1, 0, 1] and d.dtype == np.uint32
    assert strsim_amd.distance_dedupe_pairs("levenshtein", col, 1, ctx=stub)[1].tolist() == [3, 5]  # the swap is two edits there
    root, label, count = strsim_amd.distance_cluster("damerau_levenshtein", col, 1, ctx=stub)
    assert stub.calls[-1] == ("damerau_levenshtein", [c for c in col if c is not None], 1)  # the nulls are dropped, never kept as ""
    assert root.tolist() == [0, 1, -1, 0, 0, 1, -1, 7] and label.tolist() == [0, 1, -1, 0, 0, 1, -1, 2] and count == 3


class _FakeLib:
    """strsim_distance_join_host as Context.distance_join calls it: the capacity protocol over a fixed result"""
    def __init__(self, result):
        self.result = result
        self.calls = []

    def strsim_distance_join_host(self, h, kind, qo, qv, nq, co, cv, nc, k, flags, capacity, indptr, index, dist, nnz):
        ip, ix, ds = self.result
        self.calls.append((capacity, index is None, flags, k, kind))
        C.memmove(indptr, ip.ctypes.data, ip.nbytes)
        C.cast(nnz, C.POINTER(C.c_uint64))[0] = ix.size
        if ix.size <= capacity and ix.size:
            C.memmove(index, ix.ctypes.data, ix.nbytes)
            C.memmove(dist, ds.ctypes.data, ds.nbytes)
        return 0


def test_context_distance_join_retries_once_with_the_exact_size(monkeypatch):
    import strsim_amd
    from strsim_amd import context
    Q, Cs = ["ab", "abc", "b"], ["ab", "abc", "abd", "b"]
    exp = R.join("osa", Q, Cs, 2)
    fake = _FakeLib(exp)
    monkeypatch.setattr(context, "lib", lambda: fake)
    ctx = context.Context.__new__(context.Context)
    ctx._h = None
    cols = (*strsim_amd.pack_strings(Q), *strsim_amd.pack_strings(Cs))
    n = exp[1].size
    assert n > 3
    got = ctx.distance_join("osa", *cols, 2, capacity=3)
    assert R.same(got, exp) and [c[0] for c in fake.calls] == [3, n] and got[2].dtype == np.uint32
    fake.calls.clear()
    assert R.same(ctx.distance_join("osa", *cols, 2), exp) and [c[0] for c in fake.calls] == [4 * 3 + 1024]  # the guess holds
    fake.calls.clear()
    assert R.same(ctx.distance_join("damerau_levenshtein", *cols, 2, True, capacity=n), exp) and fake.calls == [(n, False, 1, 2, 2)]
    fake.calls.clear()
    assert np.array_equal(ctx.distance_join("levenshtein", *cols, None, count_only=True), exp[0]) and fake.calls == [(0, True, 0, UNBOUNDED, 0)]


# ---- the frames of the GPU tests --------------------------------------------------------------------------------------------------

def test_distance_join_gpu_frames_are_not_vacuous():
    # every parity frame of tests/test_distance_join_gpu.py at every k it is run at: 0 < nnz < the pairs on the reference side
    import distance_join_frames as F
    for measure in MEASURES:
        for k in (0, 1, 2, 3):
            assert F.not_vacuous(F.known_matrix(measure), k), (measure, k)
            B = F.boundary_matrix(measure)
            assert F.not_vacuous(B, k) and F.not_vacuous(B, k, True), (measure, k)
        M = F.near_matrix(measure)
        for nq in F.GEOMETRY_NQ:
            for nc in F.GEOMETRY_NC:
                for upper in (False, True):
                    for k in F.geometry_ks(nq, nc):
                        assert F.not_vacuous(M[:nq, :nc], k, upper), (measure, nq, nc, upper, k)
    Q, Cs = F.boundary()
    assert {len(s.encode()) for s in Q} >= {0, 1, 31, 32, 33} and {len(s.encode()) for s in Cs} >= {0, 1, 31, 32, 33}
    assert any(not s.isascii() and len(s.encode()) <= 32 for s in Q) and any(not s.isascii() and len(s.encode()) <= 32 for s in Cs)
    assert any(s.isascii() and len(s) == 33 for s in Q) and any(s.isascii() and len(s) == 33 for s in Cs)
    lq, lc = np.array([len(s) for s in Q]), np.array([len(s) for s in Cs])
    gap = np.abs(lq[:, None] - lc[None, :])
    for measure in MEASURES:
        B = F.boundary_matrix(measure)
        for k in (0, 1, 2, 3):
            assert (gap == k).any() and (gap == k + 1).any() and (B == k).any() and (B == k + 1).any(), (measure, k)
    # a 32-byte candidate against 32-byte queries that the OSA distance leaves undecided
    U = F.undecided(F.boundary_matrix("osa"), lq, lc, 2)
    assert U[np.ix_(lq == 32, lc == 32)].any()


@pytest.mark.parametrize("k", [2, 3])
def test_distance_join_gpu_damerau_frames_exercise_the_filter(k):
    # at least 20 hits with dl < osa <= 2 k, at least 20 undecided pairs that are no hits, and a whole wave of queries in length
    # order that leaves nothing undecided (so that a sweep runs without the cell DP beside sweeps that run it)
    import distance_join_frames as F
    for X in (F.near_duplicates(), F.cluster_column()):
        below, misses, quiet = F.damerau_frame_report(X, k)
        assert below >= 20 and misses >= 20, (len(X), k, below, misses)
    assert F.damerau_frame_report(F.near_duplicates(), k)[2] >= 1
    Q, Cs = F.boundary()
    ascii_lane = lambda X: [s for s in X if s.isascii() and len(s) <= 32]
    O, D = R.matrix("osa", ascii_lane(Q), ascii_lane(Cs)), R.matrix("damerau_levenshtein", ascii_lane(Q), ascii_lane(Cs))
    assert ((D <= k) & (D < O)).any()


# ---- the plugin's surfaces ------------------------------------------------------------------------------------------------------

def test_distance_join_plugin_symbols_and_polars_wrapper_source(L):
    plug = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    for kind in MEASURES:
        for family in ("distance_join_", "distance_cluster_"):
            assert getattr(L, "_polars_plugin_" + family + kind) is not None and getattr(L, "_polars_plugin_field_" + family + kind) is not None
            assert "POLARS_PLUGIN_DECLARE(%s%s)" % (family, kind) in plug
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    compile(src, "polars_strsim/__init__.py", "exec")
    assert '__all__ += ["distance_join", "distance_cluster"]' in src
    assert ('def distance_join(expr: IntoExpr, candidates: IntoExpr, measure: str = "levenshtein", max_distance: int | None = None)'
            ' -> pl.Expr:') in src
    assert 'def distance_cluster(expr: IntoExpr, measure: str = "levenshtein", max_distance: int | None = None) -> pl.Expr:' in src
    body = src[src.index("def _distance_join_measure("):]
    for word in ("is_elementwise=False", '"distance_join_" + measure', '"distance_cluster_" + measure', "pl.lit(max_distance, dtype=pl.UInt32)",
                 "max_distance is required"):
        assert word in body, word


@pytest.mark.parametrize("kind", MEASURES)
def test_distance_join_plugin_fields(kind):
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    want = pa.large_list(pa.field("item", pa.struct([pa.field("index", pa.uint32()), pa.field("distance", pa.uint32())])))
    assert arrow_host.field_plugin("distance_join_" + kind, ("queries", "cands", "max_distance")) == ("queries", want)
    assert arrow_host.field_plugin("distance_cluster_" + kind, ("name", "max_distance")) == ("name", pa.uint32())


def test_distance_join_plugin_argument_errors_need_no_device():
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host as H
    u32 = lambda v: pa.array([v], type=pa.uint32())
    LIST = pa.large_list(pa.field("item", pa.struct([pa.field("index", pa.uint32()), pa.field("distance", pa.uint32())])))
    for extra, words in (([u32(1), u32(1)], "distance_join: expected 2 input series .*got 4"),
                         ([pa.array([2.0], type=pa.float64())], "max_distance must be a UInt32 series, got Arrow format 'g'"),
                         ([pa.array([1, 2], type=pa.uint32())], "max_distance must be a single value, got 2 rows")):
        with pytest.raises(H.PluginError, match=words):
            H.call_plugin("distance_join_osa", ["abc"], ["abd"], out_type=LIST, extra=extra)
    for b, extra, words in ((u32(2), [u32(0)], "distance_cluster: expected 2 input series .*got 3"),
                            (pa.array([None], type=pa.uint32()), [], "max_distance must not be null"),
                            (pa.array([0.5]), [], "max_distance must be a UInt32 series, got Arrow format 'g'")):
        with pytest.raises(H.PluginError, match=words):
            H.call_plugin("distance_cluster_damerau_levenshtein", ["abc", "abd"], b, out_type=pa.uint32(), extra=extra)
