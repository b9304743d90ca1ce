"""Bounded edit distances without a GPU: the references against the known answers and each other, the host builds of the lane
recurrence and of the block-cutoff column step (strsim_distance.h) against them, the argument checks of strsim_distance_device /
_host, and the plugin's field functions."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import distance_ref as R
import osa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "distance_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
U = R.UNBOUNDED
MEASURES = ("levenshtein", "osa")


@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="dist_harness_")
    so = os.path.join(d.name, "libdist_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    L.dist_lane_distance.restype = C.c_uint32
    L.dist_lane_distance.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint32]
    L.dist_lane_class.restype = C.c_uint32
    L.dist_lane_class.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]
    L.dist_block_distance.restype = C.c_uint32
    L.dist_block_distance.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]
    yield L
    d.cleanup()


@pytest.fixture(scope="module")
def cdist():
    return R.CDist()


def _block(H, measure, a, b, k):
    x = np.array([ord(c) for c in a] or [0], dtype=np.uint32)
    y = np.array([ord(c) for c in b] or [0], dtype=np.uint32)
    cols, words = C.c_uint64(0), C.c_uint64(0)
    d = H.dist_block_distance(x.ctypes.data, len(a), y.ctypes.data, len(b), 1 if measure == "osa" else 0, k, C.byref(cols),
                              C.byref(words))
    return d, cols.value


def _edits(rng, s, alphabet, n):
    t = list(s)
    for _ in range(n):
        op = rng.randrange(4)
        if op == 0 and t:
            t[rng.randrange(len(t))] = rng.choice(alphabet)
        elif op == 1:
            t.insert(rng.randint(0, len(t)), rng.choice(alphabet))
        elif op == 2 and t:
            del t[rng.randrange(len(t))]
        elif op == 3 and len(t) >= 2:
            i = rng.randrange(len(t) - 1)
            t[i], t[i + 1] = t[i + 1], t[i]
    return "".join(t)


@pytest.mark.parametrize("a,b,lev,osa", R.KNOWN)
def test_dist_known_answers(cdist, a, b, lev, osa):
    for m, want in (("levenshtein", lev), ("osa", osa)):
        assert R.distance(m, a, b) == want and R.distance(m, b, a) == want
        assert cdist.distance(m, a, b) == want
        assert R.batch_numpy(m, [a], [b]).tolist() == [want]
        for k in (0, 1, 2, 5):
            assert R.distance(m, a, b, k) == (want if want <= k else k + 1)
    assert osa_ref.distance(a, b) == osa


def test_dist_references_agree(cdist):
    rng = random.Random(12)
    A, B = [], []
    for _ in range(800):
        a = "".join(rng.choice("abcü東") for _ in range(rng.randint(0, 14)))
        A.append(a)
        B.append(_edits(rng, a, "abcü東", rng.randint(0, 4)))
    for m in MEASURES:
        for k in (None, 0, 2):
            got = R.batch_numpy(m, A, B, k)
            for a, b, g in zip(A, B, got):
                assert g == R.distance(m, a, b, k) == cdist.distance(m, a, b, k), (m, a, b, k)
    # the band is exact within it
    for _ in range(20):
        a = "".join(rng.choice("xyz") for _ in range(rng.randint(100, 300)))
        b = _edits(rng, a, "xyz", rng.randint(0, 6))
        for m in MEASURES:
            assert cdist.distance(m, a, b, band=20) == cdist.distance(m, a, b)


def _pair(rng, lp, lt):
    p = "".join(rng.choice("abc") for _ in range(lp))
    t = list(_edits(rng, p, "abc", rng.randint(0, 3)))
    t = (t + [rng.choice("abc") for _ in range(64)])[:lt]
    return p, "".join(t)


@pytest.mark.parametrize("measure", MEASURES)
def test_dist_lane_every_length_pair(H, measure):
    """Pattern 0..64 x text 0..64 bytes (pattern = the longer string, as in k_dist_lane), k in {0, 1, 3, 64, unbounded}."""
    rng = random.Random(640)
    P, T = [], []
    for lp in range(65):
        for lt in range(lp + 1):
            p, t = _pair(rng, lp, lt)
            P.append(p)
            T.append(t)
    want = R.batch_numpy(measure, P, T)
    tr = 1 if measure == "osa" else 0
    for p, t, d in zip(P, T, want.tolist()):
        tmax = min(64, len(t) + rng.randint(0, 8))
        for k in (0, 1, 3, 64, U):
            w = R.clamp(d, k)
            assert H.dist_lane_distance(p.encode(), len(p), t.encode(), len(t), tmax, 1, tr, k) == w, (p, t, k)
            if len(p) <= 32:
                assert H.dist_lane_distance(p.encode(), len(p), t.encode(), len(t), tmax, 0, tr, k) == w, (p, t, k)


def test_dist_lane_row_classes(H):
    """k_dist_lane's split of the rows: past the end, to the wave tier (longer than 64 bytes or not ASCII), cut by the length
    prefilter (lengths differ by more than k), or run in the lane."""
    NONE, WAVE, CUT, RUN = 0, 1, 2, 3
    for k in (0, 1, 3, 64, U):
        for la in (0, 1, 5, 32, 63, 64, 65, 200):
            for lb in (0, 1, 4, 33, 64, 65, 1000):
                assert H.dist_lane_class(0, la, lb, 1, k) == NONE
                fits = la <= 64 and lb <= 64
                assert H.dist_lane_class(1, la, lb, 0, k) == WAVE
                want = WAVE if not fits else (CUT if abs(la - lb) > k else RUN)
                assert H.dist_lane_class(1, la, lb, 1, k) == want, (la, lb, k)


@pytest.mark.parametrize("measure", MEASURES)
def test_dist_block_cutoff_word_boundaries(H, cdist, measure):
    """The block-cutoff column step on patterns and texts crossing 63/64/65 and 127/128/129 values, near and far pairs, small k."""
    rng = random.Random(129)
    lens = (1, 2, 63, 64, 65, 127, 128, 129, 130, 200)
    for la in lens:
        for lb in lens:
            for alphabet in ("ab", "abcdefgh"):
                a = "".join(rng.choice(alphabet) for _ in range(la))
                near = _edits(rng, a, alphabet, rng.randint(0, 5))
                near = (near + "".join(rng.choice(alphabet) for _ in range(lb)))[:lb]
                far = "".join(rng.choice(alphabet) for _ in range(lb))
                for b in (near, far):
                    d = cdist.distance(measure, a, b)
                    for k in (0, 1, 2, 3, 5, 8, 63, 64, 65, 100, U):
                        got, _ = _block(H, measure, a, b, k)
                        assert got == R.clamp(d, k), (measure, a, b, k, d)


@pytest.mark.parametrize("measure", MEASURES)
def test_dist_block_cutoff_random_edits(H, cdist, measure):
    rng = random.Random(7)
    for _ in range(600):
        alphabet = rng.choice(["ab", "abc", "acgt", "etaoinshrdlu", "aé東😀"])
        a = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 300)))
        b = _edits(rng, a, alphabet, rng.randint(0, 12))
        d = cdist.distance(measure, a, b)
        for k in (0, 1, 2, 4, 7, 16, 70, U):
            got, _ = _block(H, measure, a, b, k)
            assert got == R.clamp(d, k), (measure, a, b, k, d)


def test_dist_block_cutoff_ends_early(H):
    """An unrelated pair is decided once word 0's bottom score reaches k + 64 (column 68 for k = 4), not at the end of the text."""
    rng = random.Random(3)
    a = "".join(rng.choice("abcdefghij") for _ in range(1000))
    b = "".join(rng.choice("klmnopqrst") for _ in range(1000))
    for m in MEASURES:
        got, cols = _block(H, m, a, b, 4)
        assert got == 5 and cols <= 64 + 4 + 1
        got, cols = _block(H, m, a, b, U)
        assert got == 1000 and cols == 1000


# ---- the C ABI's argument checks (no device: each returns before it looks at the context) ----

@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    vp, u64 = C.c_void_p, C.c_uint64
    for name in ("strsim_distance_device", "strsim_distance_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, C.c_uint32, vp, u64]
    L.strsim_last_error_message.restype = C.c_char_p
    L.strsim_abi_version.restype = C.c_uint32
    return L


@pytest.mark.parametrize("entry", ["strsim_distance_device", "strsim_distance_host"])
def test_dist_argument_errors_without_a_device(L, entry):
    f = getattr(L, entry)
    off = np.array([0, 1, 2], dtype=np.uint32)
    val = np.frombuffer(b"ab", dtype=np.uint8).copy()
    out = np.zeros(2, dtype=np.uint32)
    o, v, p = off.ctypes.data, val.ctypes.data, out.ctypes.data
    for m in (-1, 1, 2, 3, 4, 5, 7, 100):  # only 0 and 6 have a distance
        assert f(None, m, o, v, 2, o, v, 2, 3, p, 2) == 2
        assert b"measure" in L.strsim_last_error_message()
    assert f(None, 0, o, v, 2, o, v, 3, U, p, 2) == 1  # shape
    assert L.strsim_last_error_message() == b"Inputs must have the same length, or one of them must be a Utf8 literal."
    assert f(None, 6, o, v, 2, o, v, 2, U, p, 3) == 2  # out_rows
    for args in ((None, v, o, v), (o, None, o, v), (o, v, None, v), (o, v, o, None)):
        assert f(None, 0, args[0], args[1], 2, args[2], args[3], 2, 1, p, 2) == 2
        assert b"NULL buffer" in L.strsim_last_error_message()
    assert f(None, 0, o, v, 2, o, v, 2, 1, None, 2) == 2
    assert f(None, 0, o, v, 2, o, v, 2, 1, p, 2) == 2  # every argument right: the NULL context
    assert b"ctx is NULL" in L.strsim_last_error_message()
    assert f(None, 6, o, v, 1, o, v, 2, 1, p, 2) == 2  # a literal on the left: shape ok, then the context
    assert f(None, 0, None, None, 0, None, None, 0, 1, None, 0) == 2  # zero rows: a no-op, but still needs a context
    assert L.strsim_abi_version() == 0x00010007


def test_dist_python_surface_without_a_device():
    import strsim_amd as S
    assert S.DISTANCE_MEASURES == ("levenshtein", "osa") and S.DISTANCE_UNBOUNDED == 0xFFFFFFFF
    assert S.MEASURES == ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice") and S.EXTRA_MEASURES == ("osa",)
    with pytest.raises(ValueError):
        S.distance("jaro", ["a"], ["b"])
    from strsim_amd.context import _max_distance
    assert _max_distance(None) == U and _max_distance(0) == 0 and _max_distance(U) == U
    for bad in (-1, U + 1):
        with pytest.raises(ValueError):
            _max_distance(bad)


@pytest.mark.parametrize("fn", ["levenshtein_distance", "osa_distance"])
def test_dist_field_is_uint32_named_after_first_input(fn):
    pytest.importorskip("pyarrow")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    from strsim_amd import arrow_host
    import pyarrow as pa
    assert arrow_host.field_plugin(fn, ("left", "right")) == ("left", pa.uint32())
    assert arrow_host.field_plugin(fn, ("q", "c", "max_distance")) == ("q", pa.uint32())
