"""Optimal string alignment (measure 6) without a GPU: the references against the known answers and each other, the host build of
the one-pair-per-lane recurrence and of the one-pair-per-wave word recurrence (strsim_osa.h) against them, strsim_measure_supported,
and the plugin's field function."""
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
    L.osa_words_distance.restype = C.c_uint64
    L.osa_words_distance.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
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


def _words_distance(lane, p, t):
    x = np.array([ord(c) for c in p] or [0], dtype=np.uint32)
    y = np.array([ord(c) for c in t] or [0], dtype=np.uint32)
    return int(lane.osa_words_distance(x.ctypes.data, len(p), y.ctypes.data, len(t)))


# pattern lengths around the 64-row words of k_dist_wave's state: one word, the last row of a word, the first of the next, three and
# four words
WORDS_PATTERN_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 200)
WORDS_ALPHABETS = ("ab\U0001F600", "abc\U00010348")  # three or four scalar values (one above 0xFFFF): matches and swaps are dense


def test_words_recurrence_across_word_boundaries(lane, cref):
    """The pattern over several 64-row words, the text from the pattern's length up to 260 values: a mutated copy of the pattern
    (adjacent swaps, substitutions, insertions up to the length drawn) or unrelated values.  Exact distances against the C DP."""
    rng = random.Random(66)
    pairs = 0
    for m in WORDS_PATTERN_LENGTHS:
        for rep in range(36):
            al = WORDS_ALPHABETS[rep & 1]
            p = [rng.choice(al) for _ in range(m)]
            n = rng.randint(m, min(260, m + 3)) if rep % 3 == 0 else rng.randint(m, 260)
            if rep % 6 == 5:
                t = [rng.choice(al) for _ in range(n)]
            else:
                t = list(p)
                for _ in range(rng.randint(0, 1 + m // 8)):
                    if len(t) >= 2:
                        i = rng.randrange(len(t) - 1)
                        t[i], t[i + 1] = t[i + 1], t[i]
                for _ in range(rng.randint(0, 1 + m // 16)):
                    t[rng.randrange(len(t))] = rng.choice(al)
                while len(t) < n:
                    t.insert(rng.randint(0, len(t)), rng.choice(al))
            p, t = "".join(p), "".join(t)
            assert _words_distance(lane, p, t) == cref.distance(p, t), (p, t)
            pairs += 1
    assert pairs == 288


# (pattern, text, distance): one case per carry between the words of a column
_X, _Y = "\U0001F600", "y"
WORDS_CARRY_CASES = [
    # tr_c: an adjacent swap whose two characters are pattern rows 63 | 64, and 127 | 128
    ("a" * 63 + _X + _Y + "a" * 64, "a" * 63 + _Y + _X + "a" * 64, 1),
    ("a" * 127 + _X + _Y + "a" * 71, "a" * 127 + _Y + _X + "a" * 71, 1),
    ("a" * 127 + _X + _Y + "a" * 71, "a" * 63 + _Y + _X + "a" * 62 + _Y + _X + "a" * 71, 3),
    # add_c: an insertion in front of a pattern of one repeated value: every row matches in every later column and the add
    # carries through whole words of matches
    ("a" * 200, _X + "a" * 200, 1),
    ("a" * 200, "a" * 100 + _X + "a" * 100, 1),
    # add_c: a match in row 61 or 62 followed by deletions up into rows 64 and 65 (the carry alone sets D0 there)
    ("a" * 61 + "b" + "aa" + "b" + "a" * 35, "a" * 58 + "b" + "a" + "b" + "aa" + "b" + "a" * 36, 3),
    # hp_c: nothing matches, D[i][j] = max(i, j): the +1 horizontal deltas of the rows above the diagonal cross every word
    ("a" * 128, "b" * 130, 130),
    # hn_c: the text's tail matches the pattern's tail after a block that matches nothing: -1 horizontal deltas in the rows
    # on both sides of 63 | 64 and 127 | 128
    ("b" + "a" * 127, "c" * 64 + "b" * 63 + "aa", 127),
    ("bb" + "c" * 128, "a" * 64 + "b" + "c" * 127, 65),
]


@pytest.mark.parametrize("case", range(len(WORDS_CARRY_CASES)))
def test_words_recurrence_carry_cases(lane, cref, case):
    a, b, d = WORDS_CARRY_CASES[case]
    p, t = (a, b) if len(a) <= len(b) else (b, a)
    assert cref.distance(p, t) == d
    assert _words_distance(lane, p, t) == d


def test_words_recurrence_known_answers(lane):
    for a, b, d, _, _ in R.KNOWN:
        p, t = (a, b) if len(a) <= len(b) else (b, a)
        assert _words_distance(lane, p, t) == d, (a, b)


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
