"""Extract (top-k by ratio / token_sort_ratio with a score cutoff) without a GPU: the exported symbols and version, argument errors
before any device, the Python surface, the plugin's field functions, the host builds of the Indel core, of the rank table and of the
sweep's window / skip / stop rules (strsim_extract.h), and the NumPy reference top-k of the GPU tests against a brute-force sort."""
import ctypes as C
import math
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import extract_ref as R
import indel_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "extract_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
ERR_ARG = 2
INF = float("inf")


def E(d, s):
    return indel_ref.normalise(d, s, 0)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    vp, u64 = C.c_void_p, C.c_uint64
    for name in ("strsim_extract_device", "strsim_extract_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, C.c_uint32, C.c_double, vp, vp]
    L.strsim_abi_version.restype = C.c_uint32
    L.strsim_last_error_message.restype = C.c_char_p
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_measure_supported.argtypes = [C.c_int, C.c_int]
    return L


@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="extract_harness_")
    so = os.path.join(d.name, "libextract_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    L.extract_core.restype = u32
    L.extract_core.argtypes = [C.c_char_p, u32, C.c_char_p, u32, C.c_int]
    L.extract_tab_nranks.restype = u32
    L.extract_tab_rank.restype = u32
    L.extract_tab_rank.argtypes = [u32, u32]
    L.extract_tab_score.restype = C.c_double
    L.extract_tab_score.argtypes = [u32]
    L.extract_tab_limit.restype = u32
    L.extract_tab_limit.argtypes = [C.c_double]
    L.extract_pair_score.restype = C.c_double
    L.extract_pair_score.argtypes = [u32, u32]
    L.extract_wave.restype = C.c_uint64
    L.extract_wave.argtypes = [vp, u32, vp, u32, vp, u32, C.c_double, vp, vp]
    L.extract_window_h.restype = None
    L.extract_window_h.argtypes = [u32, u32, C.c_double, vp]
    yield L
    d.cleanup()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

def test_extract_keeps_abi_version_1_7(L):
    assert L.strsim_abi_version() == 0x00010007
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    assert re.search(r"#define STRSIM_ABI_VERSION 0x00010007u", hdr)
    assert re.search(r"#define STRSIM_EXTRACT_MAX_K 16u", hdr)
    for name in ("strsim_extract_device", "strsim_extract_host"):
        assert re.search(r"STRSIM_API int " + name + r"\(strsim_ctx_t \*ctx, int scorer,", hdr)
    assert "strsim_measure_supported does not describe these two entry points).  `scorer`" in hdr


def test_extract_symbols_are_exported(L):
    for name in ("strsim_extract_device", "strsim_extract_host", "_polars_plugin_extract_ratio", "_polars_plugin_extract_token_sort_ratio",
                 "_polars_plugin_field_extract_ratio", "_polars_plugin_field_extract_token_sort_ratio"):
        assert getattr(L, name) is not None
    hdr = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    assert "POLARS_PLUGIN_DECLARE(extract_ratio)" in hdr and "POLARS_PLUGIN_DECLARE(extract_token_sort_ratio)" in hdr


def test_extract_leaves_measure_supported_alone(L):
    # extract is its own entry point and is not described there: best match (entry 1) still refuses the ratio family, and
    # there is no entry 3
    for m in (8, 10, 14, 16):
        assert L.strsim_measure_supported(m, 1) == 0 and L.strsim_measure_supported(m, 0) == 1
    for m in range(5):
        assert L.strsim_measure_supported(m, 1) == 1
    for m in range(-1, 18):
        assert L.strsim_measure_supported(m, 3) == 0


def _extract_call(L, name, k=1, q_rows=1, c_rows=1, scorer=8, cutoff=-INF, null_q=False, null_out=False, null_c=False, null_cv=False):
    qo = (C.c_uint32 * 2)(0, 1)
    qv = (C.c_uint8 * 1)(97)
    idx = (C.c_uint32 * 32)()
    score = (C.c_double * 32)()
    f = getattr(L, name)
    return f(None, scorer, None if null_q else C.addressof(qo), C.addressof(qv), q_rows, None if null_c else C.addressof(qo),
             None if null_cv else C.addressof(qv), c_rows, k, cutoff, None if null_out else C.addressof(idx),
             None if null_out else C.addressof(score))


@pytest.mark.parametrize("name", ["strsim_extract_device", "strsim_extract_host"])
@pytest.mark.parametrize("case,kw,msg", [
    ("k0", dict(k=0), "k=0 is outside 1..16"),
    ("k17", dict(k=17), "k=17 is outside 1..16"),
    ("scorer0", dict(scorer=0), "scorer 0"),
    ("scorer6", dict(scorer=6), "scorer 6"),
    ("scorer10", dict(scorer=10), "scorer 10"),
    ("scorer16", dict(scorer=16), "scorer 16"),
    ("scorer5", dict(scorer=5), "scorer 5"),
    ("scorer-1", dict(scorer=-1), "scorer -1"),
    ("nan_cutoff", dict(cutoff=float("nan")), "score_cutoff is NaN"),
    ("null_queries", dict(null_q=True), "NULL"),
    ("null_outputs", dict(null_out=True), "NULL"),
    ("null_candidates", dict(null_c=True), "NULL"),
    ("null_candidate_values", dict(null_cv=True), "NULL"),
    ("too_many_candidates", dict(c_rows=2 ** 32 - 1), "candidates"),
    ("too_many_queries", dict(q_rows=2 ** 32), "queries"),
])
def test_extract_argument_errors_need_no_device(L, name, case, kw, msg):
    # the arguments are checked before the context: STRSIM_ERR_ARG, with the reason in the message, on a box without a GPU
    assert _extract_call(L, name, **kw) == ERR_ARG
    text = L.strsim_last_error_message().decode()
    assert text.startswith(name + ": ") and msg in text
    if case.startswith("scorer"):
        assert "STRSIM_INDEL = 8" in text and "STRSIM_TOKEN_SORT_RATIO = 14" in text


@pytest.mark.parametrize("name", ["strsim_extract_device", "strsim_extract_host"])
@pytest.mark.parametrize("scorer", [8, 14])
@pytest.mark.parametrize("kw", [dict(), dict(k=16, cutoff=0.5), dict(cutoff=1.5), dict(q_rows=0, null_q=True, null_out=True),
                                dict(c_rows=0, null_c=True, null_cv=True)])
def test_extract_null_context_is_checked_last(L, name, scorer, kw):
    assert _extract_call(L, name, scorer=scorer, **kw) == ERR_ARG
    assert "ctx is NULL" in L.strsim_last_error_message().decode()


# ---- Python surface and plugin fields ---------------------------------------------------------------------------------------

def test_extract_python_surface():
    import strsim_amd
    from strsim_amd.context import Context
    assert "extract" in strsim_amd.__all__ and "EXTRACT_SCORERS" in strsim_amd.__all__ and callable(strsim_amd.extract)
    assert strsim_amd.EXTRACT_SCORERS == ("ratio", "token_sort_ratio")
    assert callable(Context.extract)
    for bad in ("jaro", "levenshtein", "partial_ratio", "token_set_ratio", "best_match", 8):
        with pytest.raises(ValueError, match=r"no extract by scorer .*\('ratio', 'token_sort_ratio'\)"):
            strsim_amd.extract(bad, ["a"], ["b"])
    # the search entry points that exist still refuse the ratio family, as before
    with pytest.raises(ValueError, match="no best match"):
        strsim_amd.best_match("indel", ["a"], ["b"])
    with pytest.raises(ValueError, match="no distance"):
        strsim_amd.nearest("indel", ["a"], ["b"])
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert re.search(r'__all__ = \[[^\]]*"sorensen_dice",\s*"extract",\s*\]', src)
    assert 'def extract(expr: IntoExpr, candidates: IntoExpr, scorer: str = "ratio", score_cutoff: float | None = None) -> pl.Expr:' in src
    body = src[src.index("def extract("):]
    for word in ("process.extractOne", "fuzz.ratio", "fuzz.token_sort_ratio", "/ 100", "lower candidate index", "is_elementwise=False",
                 '"extract_" + scorer', "pl.lit(score_cutoff, dtype=pl.Float64)"):
        assert word in body, word


@pytest.mark.parametrize("fn", ["extract_ratio", "extract_token_sort_ratio"])
def test_extract_field_is_index_score_struct_named_after_first_input(fn):
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    want = pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])
    assert arrow_host.field_plugin(fn, ("queries", "cands")) == ("queries", want)
    assert arrow_host.field_plugin(fn, ("q", "c", "score_cutoff")) == ("q", want)


# ---- the Indel core ---------------------------------------------------------------------------------------------------------

def _rand(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


@pytest.mark.parametrize("alphabet,planes", [("ab", 5), ("ab", 7), ("abcdefgh", 5), ("abcdefgh", 7), ("aB1 ~bA", 7)])
def test_extract_core_every_length_pair(H, alphabet, planes):
    # the uniform-text core of k_extract_lane against indel_ref.distance, query and candidate lengths 0..32 (five planes only
    # where bits 5 and 6 do not vary, as the kernel chooses)
    rng = random.Random(len(alphabet) * 10 + planes)
    bad = []
    for lq in range(33):
        for lc in range(33):
            a, b = _rand(rng, lq, alphabet), _rand(rng, lc, alphabet)
            if lc and lq and rng.random() < 0.3:
                b = (a[:lc] + b)[:lc]  # near copies: small distances
            got = H.extract_core(a.encode(), lq, b.encode(), lc, planes)
            if got != indel_ref.distance(a, b):
                bad.append((a, b, got))
    assert not bad, bad[:5]


def test_extract_core_counts_nul_bytes_as_characters(H):
    # a NUL byte is a character like any other on either side; the zero padding above the pattern's rows must not match it into
    # a counted row (seven planes: NUL differs from letters in bits 5 / 6)
    rng = random.Random(5)
    cases = [("a\0b", "a\0b"), ("\0", ""), ("", "\0\0"), ("\0", "\0\0\0"), ("ab", "a\0b\0"), ("a\0", "\0a"), ("\0" * 32, "\0" * 31),
             ("a" * 31 + "\0", "\0" + "a" * 31)]
    for _ in range(300):
        cases.append((_rand(rng, rng.randrange(33), "a\0b"), _rand(rng, rng.randrange(33), "a\0b")))
    for a, b in cases:
        assert H.extract_core(a.encode(), len(a), b.encode(), len(b), 7) == indel_ref.distance(a, b), (a, b)


def test_extract_core_known_answers(H):
    for a, b, l, d in indel_ref.KNOWN:
        if len(a) <= 32 and len(b) <= 32 and a.isascii() and b.isascii():
            assert H.extract_core(a.encode(), len(a), b.encode(), len(b), 7) == d


# ---- the rank table ---------------------------------------------------------------------------------------------------------

def _attainable():
    return [(d, s) for s in range(1, 65) for d in range(s % 2, s + 1, 2)]


def test_extract_rank_order_is_the_order_of_the_f64_scores(H):
    pairs = _attainable()
    assert len(pairs) == 1088
    every = pairs + [(d, s) for s in range(0, 65) for d in range(s + 1)]
    score = {p: E(*p) for p in every}
    rank = {p: H.extract_tab_rank(*p) for p in every}
    n = H.extract_tab_nranks()
    assert len({score[p] for p in pairs}) == 631
    assert n == len(set(score.values())) and max(rank.values()) == n - 1
    assert rank[(0, 0)] == 0 and rank[(0, 64)] == 0 and rank[(5, 5)] == n - 1
    # the f64 score orders pairs exactly as the rational d / s does, and the rank is that order reversed
    from fractions import Fraction
    for p in every:
        assert H.extract_pair_score(*p) == score[p] == H.extract_tab_score(rank[p])
    order = sorted(every, key=lambda p: (Fraction(p[0], p[1]) if p[1] else Fraction(0), p))
    for a, b in zip(order, order[1:]):
        fa, fb = (Fraction(*p) if p[1] else Fraction(0) for p in (a, b))
        if fa == fb:
            assert score[a] == score[b] and rank[a] == rank[b]
        else:
            assert score[a] > score[b] and rank[a] < rank[b]
    scores = [H.extract_tab_score(r) for r in range(n)]
    assert scores[0] == 1.0 and scores[-1] == 0.0 and all(x > y for x, y in zip(scores, scores[1:]))


def test_extract_cutoff_to_rank_limit_agrees_with_score_ge_cutoff(H):
    n = H.extract_tab_nranks()
    scores = [H.extract_tab_score(r) for r in range(n)]
    cuts = [-INF, INF, 0.0, -0.0, 1.0, 1.5, -1.0, 0.5, 5e-324]
    for v in scores:
        cuts += [v, math.nextafter(v, INF), math.nextafter(v, -INF)]
    for c in cuts:
        assert H.extract_tab_limit(c) == sum(1 for v in scores if v >= c), c
    assert H.extract_tab_limit(-INF) == n and H.extract_tab_limit(0.0) == n and H.extract_tab_limit(1.0) == 1
    assert H.extract_tab_limit(math.nextafter(1.0, INF)) == 0 and H.extract_tab_limit(1.5) == 0


# ---- the sweep --------------------------------------------------------------------------------------------------------------

def _window(H, lmin, lmax, cutoff):
    out = (C.c_uint32 * 2)()
    H.extract_window_h(lmin, lmax, cutoff, C.addressof(out))
    return out[0], out[1]


@pytest.mark.parametrize("cutoff", [-INF, 0.0, 0.25, 0.5, E(2, 6), 0.8, 0.9, 1.0])
def test_extract_window_is_exactly_the_admissible_lengths(H, cutoff):
    # the lengths some query of the wave can need under the cutoff alone: ub(lq, lc) = E(|lq - lc|, lq + lc) >= cutoff
    for lmin in range(33):
        for lmax in range(lmin, min(lmin + 3, 33)):
            need = [lc for lc in range(33) if any(E(abs(lq - lc), lq + lc) >= cutoff for lq in range(lmin, lmax + 1))]
            assert _window(H, lmin, lmax, cutoff) == (need[0], need[-1]), (lmin, lmax)
            assert need == list(range(need[0], need[-1] + 1))
    assert _window(H, 3, 3, 1.5) == (0xFFFFFFFF, 0xFFFFFFFF)


def _wave(H, qlen, clen, dist, K, cutoff):
    nq, nc = len(qlen), len(clen)
    ql = np.ascontiguousarray(qlen, dtype=np.uint32)
    cl = np.ascontiguousarray(clen, dtype=np.uint32)
    dm = np.ascontiguousarray(dist, dtype=np.uint32)
    oi = np.zeros((nq, K), dtype=np.uint32)
    osc = np.zeros((nq, K), dtype=np.float64)
    visited = H.extract_wave(ql.ctypes.data, nq, cl.ctypes.data, nc, dm.ctypes.data, K, -INF if cutoff is None else cutoff,
                             oi.ctypes.data, osc.ctypes.data)
    return np.where(oi == 0xFFFFFFFF, -1, oi.astype(np.int64)), osc, visited


def _scores(qlen, clen, dist):
    s = (np.asarray(qlen)[:, None] + np.asarray(clen)[None, :]).astype(np.int64)
    return indel_ref.scores_from_distances(np.asarray(dist).ravel(), s.ravel(), np.zeros(s.size, dtype=np.int64)).reshape(s.shape)


def _same(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


CUTOFFS = [None, 0.0, 0.5, math.nextafter(E(2, 6), -INF), E(2, 6), math.nextafter(E(2, 6), INF), 1.0, 1.5]


@pytest.mark.parametrize("seed", range(12))
def test_extract_sweep_rules_match_brute_force(H, seed):
    # one wave's sweep with the window, skip and stop rules against a full sort, on distances |lq - lc| <= d <= lq + lc of the
    # right parity with many ties; over the seeds, pruning must have skipped candidates
    rng = np.random.default_rng(seed)
    lbase = int(rng.integers(0, 33))
    nq = int(rng.integers(1, 65))
    qlen = np.clip(lbase + rng.integers(0, 2, size=nq), 0, 32)
    nc = int(rng.integers(1, 300))
    clen = rng.integers(0, 33, size=nc)
    gap = np.abs(qlen[:, None] - clen[None, :])
    room = np.minimum(qlen[:, None], clen[None, :])  # d = gap + 2 * (min - lcs)
    near = rng.integers(0, 2, size=(nq, nc))
    dist = gap + 2 * np.where(near, np.minimum(room, rng.integers(0, 3, size=(nq, nc))), rng.integers(0, 33, size=(nq, nc)) % (room + 1))
    sc = _scores(qlen, clen, dist)
    skipped = 0
    for K in (1, 4, 16):
        for cutoff in CUTOFFS:
            idx, val, visited = _wave(H, qlen, clen, dist, K, cutoff)
            ri, rv = R.brute_topk(sc, K, cutoff)
            assert np.array_equal(idx, ri), (K, cutoff)
            assert _same(val, rv), (K, cutoff)
            assert visited <= nc
            skipped += nc - visited
    assert skipped > 0


def test_extract_sweep_prunes_by_window_and_by_the_running_bound(H):
    # query length 4; candidates of lengths 1, 4, 4, 8, 20
    qlen, clen = np.array([4]), np.array([1, 4, 4, 8, 20])
    dist = np.array([[3, 0, 2, 4, 16]])
    # K = 1: the exact match at the query's own length (rank 0) ends the sweep before any other length
    idx, val, visited = _wave(H, qlen, clen, dist, 1, None)
    assert idx.tolist() == [[1]] and val.tolist() == [[1.0]] and visited == 2
    # a cutoff of 0.5 admits lengths 2..12 only (ub(4, 1) = 0.4, ub(4, 20) = 1/3): two candidates are never visited
    idx, val, visited = _wave(H, qlen, clen, dist, 16, 0.5)
    assert idx[0, :4].tolist() == [1, 2, 3, -1] and val[0, :3].tolist() == [1.0, 0.75, E(4, 12)] and visited == 3
    # no cutoff and room in the list: everything is visited and reported, the empty slots after it
    idx, val, visited = _wave(H, qlen, clen, dist, 16, None)
    assert idx[0, :6].tolist() == [1, 2, 3, 0, 4, -1] and visited == 5


def test_extract_sweep_admits_a_cross_length_tie_with_a_lower_index(H):
    # "ab" against "abxxxx" (d 4, s 8, index 0) and "ba" (d 2, s 4, index 1): both 0.5; the own length is visited first, the
    # list is then full with the bound 0.5, and length 6 (ub = E(4, 8) = 0.5, a tie) must still be visited and win by its index
    qlen, clen = np.array([2]), np.array([6, 2])
    idx, val, visited = _wave(H, qlen, clen, np.array([[4, 2]]), 1, None)
    assert idx.tolist() == [[0]] and val.tolist() == [[0.5]] and visited == 2
    # the other way round the tie loses, whichever is visited first
    idx, val, _ = _wave(H, qlen, np.array([2, 6]), np.array([[2, 4]]), 1, None)
    assert idx.tolist() == [[0]] and val.tolist() == [[0.5]]
    # one length further out (ub(2, 7) = E(5, 9) < 0.5) is not visited once the list is full at 0.5
    idx, val, visited = _wave(H, qlen, np.array([7, 2]), np.array([[5, 2]]), 1, None)
    assert idx.tolist() == [[1]] and visited == 1


def test_extract_sweep_empty_strings(H):
    # (0, 0) scores 1.0; (0, n > 0) scores 0.0 and is reported only under a cutoff <= 0
    qlen, clen = np.array([0]), np.array([3, 0, 1])
    dist = np.array([[3, 0, 1]])
    idx, val, _ = _wave(H, qlen, clen, dist, 4, None)
    assert idx.tolist() == [[1, 0, 2, -1]] and val[0, :3].tolist() == [1.0, 0.0, 0.0]
    idx, val, _ = _wave(H, qlen, clen, dist, 4, 0.0)
    assert idx.tolist() == [[1, 0, 2, -1]]
    idx, val, visited = _wave(H, qlen, clen, dist, 4, 5e-324)
    assert idx.tolist() == [[1, -1, -1, -1]] and visited == 1


# ---- the NumPy reference --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_extract_reference_topk_matches_a_brute_force_sort(seed):
    rng = np.random.default_rng(seed)
    n, m = 7, int(rng.integers(0, 40))
    sc = rng.integers(0, 5, size=(n, m)) / 4.0  # many ties
    for k in (1, 3, 16):
        for cut in (None, 0.0, 0.25, 0.5, 1.0, 1.5):
            a = R.topk(sc, k, cut)
            b = R.brute_topk(sc, k, cut)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def test_extract_reference_score_matrix():
    q, c = ["ab", "", "b a"], ["ba", "abxxxx", "", "a  b"]
    M = R.score_matrix("ratio", q, c)
    assert M[0].tolist() == [0.5, 0.5, 0.0, E(2, 6)] and M[1].tolist() == [0.0, 0.0, 1.0, 0.0]
    T = R.score_matrix("token_sort_ratio", q, c)
    assert T[2, 3] == 1.0 and T[2, 0] == E(3, 5) and T[1, 2] == 1.0
    import token_ref
    for i, a in enumerate(q):
        for j, b in enumerate(c):
            assert T[i, j] == token_ref.token_sort_ratio(a, b) and M[i, j] == indel_ref.score(a, b)
    A, B = token_ref.gen_frame(3, 40)
    T2 = R.score_matrix("token_sort_ratio", A, B)
    assert all(T2[i, j] == token_ref.token_sort_ratio(A[i], B[j]) for i in range(0, 40, 3) for j in range(40))
    # the form for a long candidate column gives the same matrix
    rng = random.Random(9)
    X = [_rand(rng, rng.randrange(0, 9), "abc ") for _ in range(5)] + ["", "héllo wörld"]
    Y = [_rand(rng, rng.randrange(0, 11), "abc ") for _ in range(400)] + ["", "wörld", "x" * 40]
    for scorer in R.SCORERS:
        assert _same(R.score_matrix(scorer, X, Y), R._few_against_many(*([token_ref.token_sort(s) for s in Z] if scorer != "ratio" else Z
                                                                        for Z in (X, Y))))
    idx, val = R.extract("ratio", q, c, 2, 0.5)
    assert idx.tolist() == [[3, 0], [2, -1], [0, -1]] and val[0].tolist() == [E(2, 6), 0.5]
