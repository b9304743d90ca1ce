"""Optimal string alignment (measure 6) without a GPU: the references against the known answers and each other, the host build of
the one-pair-per-lane recurrence (strsim_osa.h) against them, strsim_measure_supported, and the plugin's field function."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import model_py as M
import osa_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "osa_lane_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")


@pytest.fixture(scope="module")
def cref():
    return R.CRef()


@pytest.fixture(scope="module")
def lane():
    d = tempfile.TemporaryDirectory(prefix="osa_lane_")
    so = os.path.join(d.name, "libosa_lane.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    L.osa_lane_distance.restype = C.c_uint32
    L.osa_lane_distance.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int]
    L.osa_lane_score.restype = C.c_double
    L.osa_lane_score.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    yield L
    d.cleanup()


@pytest.mark.parametrize("a,b,d,d_lev,s", R.KNOWN)
def test_known_answers(cref, a, b, d, d_lev, s):
    assert R.distance(a, b) == d and R.distance(b, a) == d
    assert cref.distance(a, b) == d
    assert R.score(a, b) == s and cref.score(a, b) == s
    assert M.levenshtein(a, b) == (1.0 if not a and not b else 1.0 - d_lev / max(len(a), len(b)))


def test_batch_numpy_matches_known_answers():
    got = R.batch_numpy([k[0] for k in R.KNOWN], [k[1] for k in R.KNOWN])
    assert got.tolist() == [k[4] for k in R.KNOWN]


def _swappy(rng, alphabet, lo, hi):
    s = list(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))
    t = list(s)
    for _ in range(rng.randint(0, 3)):
        if len(t) >= 2:
            i = rng.randrange(len(t) - 1)
            t[i], t[i + 1] = t[i + 1], t[i]
    if t and rng.random() < 0.3:
        t[rng.randrange(len(t))] = rng.choice(alphabet)
    if rng.random() < 0.2:
        t.insert(rng.randint(0, len(t)), rng.choice(alphabet))
    return "".join(s), "".join(t)


def test_references_agree_symmetric_and_below_levenshtein(cref):
    rng = random.Random(6)
    A, B = [], []
    for _ in range(1500):
        a, b = _swappy(rng, "abcü", 0, 12)
        A.append(a)
        B.append(b)
    np_scores = R.batch_numpy(A, B)
    for a, b, s in zip(A, B, np_scores):
        d = R.distance(a, b)
        assert d == R.distance(b, a) == cref.distance(a, b)
        assert R.score(a, b) == s
        assert R.score(a, b) >= M.levenshtein(a, b)  # same denominator: d_osa <= d_lev


def test_c_reference_on_long_strings_matches_python(cref):
    rng = random.Random(7)
    for _ in range(5):
        a, b = _swappy(rng, "xyz", 150, 300)
        assert cref.distance(a, b) == R.distance(a, b)


def test_lane_recurrence_every_length_pair(lane):
    """Pattern 0..64 x text 0..64 bytes, 64-bit masks (and 32-bit ones up to 32), columns run beyond the text as in a wave."""
    rng = random.Random(64)
    for lp in range(65):
        for lt in range(65):
            p = "".join(rng.choice("ab") for _ in range(lp))
            t = list(p[:lt]) + [rng.choice("ab") for _ in range(lt - min(lp, lt))]
            for _ in range(rng.randint(0, 4)):
                if len(t) >= 2:
                    i = rng.randrange(len(t) - 1)
                    t[i], t[i + 1] = t[i + 1], t[i]
            t = "".join(t)
            want = R.distance(p, t)
            tmax = min(64, lt + rng.randint(0, 8))
            assert lane.osa_lane_distance(p.encode(), lp, t.encode(), lt, tmax, 1) == want, (p, t)
            if lp <= 32:
                assert lane.osa_lane_distance(p.encode(), lp, t.encode(), lt, tmax, 0) == want, (p, t)


def test_lane_recurrence_random_transpositions(lane):
    rng = random.Random(65)
    alphabet = [chr(c) for c in range(1, 128)]
    for _ in range(4000):
        a, b = _swappy(rng, rng.choice(["ab", "abc", "etaoinshrdlu", alphabet]), 0, 64)
        a, b = a[:64], b[:64]
        p, t = (a, b) if len(a) >= len(b) else (b, a)
        d = lane.osa_lane_distance(p.encode(), len(p), t.encode(), len(t), len(t), 1)
        assert d == R.distance(a, b), (a, b)
        assert lane.osa_lane_score(d, len(a), len(b)) == R.score(a, b)


def test_lane_recurrence_known_answers(lane):
    for a, b, d, _, s in R.KNOWN:
        if all(ord(c) < 128 for c in a + b) and len(a) <= 64 and len(b) <= 64:
            for p, t in ((a, b), (b, a)):
                assert lane.osa_lane_distance(p.encode(), len(p), t.encode(), len(t), len(t), 1) == d


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_measure_supported.argtypes = [C.c_int, C.c_int]
    return L


PAIRWISE, BEST_MATCH, CODEC = 0, 1, 2


def test_measure_supported(L):
    for m in range(5):
        for e in (PAIRWISE, BEST_MATCH, CODEC):
            assert L.strsim_measure_supported(m, e) == 1, (m, e)
    assert L.strsim_measure_supported(6, PAIRWISE) == 1
    assert L.strsim_measure_supported(6, BEST_MATCH) == 0
    assert L.strsim_measure_supported(6, CODEC) == 0
    for m in (-1, 5, 7):
        for e in (PAIRWISE, BEST_MATCH, CODEC):
            assert L.strsim_measure_supported(m, e) == 0, (m, e)
    assert L.strsim_measure_supported(0, 3) == 0


def test_measure_supported_from_python():
    import strsim_amd as S
    assert S.MEASURES == ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")
    assert S.EXTRA_MEASURES == ("osa",) and S.MEASURE_ID["osa"] == 6
    assert S.measure_supported("osa") and not S.measure_supported("osa", "best_match") and not S.measure_supported("osa", "codec")


def test_osa_errors_before_any_device(L):
    """A NULL context is an argument error for OSA as for the five; best match and the codec refuse measure 6 without a device."""
    vp, u64 = C.c_void_p, C.c_uint64
    L.strsim_pairs_device.restype = C.c_int
    L.strsim_pairs_device.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, vp, u64]
    L.strsim_best_match_host.restype = C.c_int
    L.strsim_best_match_host.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, C.c_uint32, C.c_double, vp, vp]
    assert L.strsim_pairs_device(None, 6, None, None, 1, None, None, 1, None, 1) == 2
    assert L.strsim_best_match_host(None, 6, None, None, 0, None, None, 0, 1, 0.0, None, None) == 2


def test_field_osa_is_float64_named_after_first_input():
    pytest.importorskip("pyarrow")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    from strsim_amd import arrow_host
    import pyarrow as pa
    name, typ = arrow_host.field_plugin("osa", ("left", "right"))
    assert name == "left" and typ == pa.float64()
