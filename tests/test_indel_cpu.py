"""Indel (LCS) similarity and distance (measure 8) without a GPU: the references against the known answers and each other, the host
build of the lane recurrence and of the wave tier's word step (strsim_indel.h) against them, strsim_measure_supported, the argument
errors of the distance entries, the Python surface and the plugin's field functions and symbols."""
import ctypes as C
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import indel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "indel_lane_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
U = 0xFFFFFFFF
INDEL = 8


@pytest.fixture(scope="module")
def cref():
    return R.CRef()


@pytest.fixture(scope="module")
def lane():
    d = tempfile.TemporaryDirectory(prefix="indel_lane_")
    so = os.path.join(d.name, "libindel_lane.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    L.indel_lane_lcs_w.restype = C.c_uint32
    L.indel_lane_lcs_w.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    L.indel_words_lcs.restype = C.c_uint32
    L.indel_words_lcs.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.indel_score.restype = C.c_double
    L.indel_score.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.indel_clamp.restype = C.c_uint32
    L.indel_clamp.argtypes = [C.c_uint64, C.c_uint32]
    L.indel_length_cut.restype = C.c_int
    L.indel_length_cut.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    yield L
    d.cleanup()


@pytest.mark.parametrize("a,b,l,d", R.KNOWN)
def test_known_answers(cref, a, b, l, d):
    assert R.lcs(a, b) == l and R.lcs(b, a) == l
    assert R.distance(a, b) == d and cref.distance(a, b) == d and cref.lcs(b, a) == l
    want = 1.0 if len(a) + len(b) == 0 else 1.0 - d / (len(a) + len(b))
    assert R.score(a, b) == want and cref.score(a, b) == want
    if (a, b) in R.KNOWN_SCORES:
        assert R.score(a, b) == R.KNOWN_SCORES[(a, b)]


def test_batch_numpy_matches_known_answers():
    A, B = [k[0] for k in R.KNOWN], [k[1] for k in R.KNOWN]
    assert R.batch_numpy_lcs(A, B).tolist() == [k[2] for k in R.KNOWN]
    assert R.batch_numpy_distance(A, B).tolist() == [k[3] for k in R.KNOWN]
    assert R.batch_numpy(A, B).tolist() == [R.score(a, b) for a, b in zip(A, B)]


def test_the_score_is_not_two_lcs_over_the_sum():
    """The issue's count: 1 - d / s and 2 l / s differ in the last bit for 8 950 of the 22 649 combinations with s < 300."""
    total = differ = 0
    for s in range(1, 300):
        for l in range(0, s // 2 + 1):
            total += 1
            differ += (1.0 - ((s - 2 * l) / s)) != (2 * l) / s
    assert (total, differ) == (22649, 8950)


def _edit(rng, alphabet, lo, hi):
    s = [rng.choice(alphabet) for _ in range(rng.randint(lo, hi))]
    t = list(s)
    for _ in range(rng.randint(0, 4)):
        op = rng.randrange(3)
        if op == 0 and t:
            del t[rng.randrange(len(t))]
        elif op == 1:
            t.insert(rng.randint(0, len(t)), rng.choice(alphabet))
        elif t:
            t[rng.randrange(len(t))] = rng.choice(alphabet)
    return "".join(s), "".join(t)


def test_references_agree_and_are_symmetric(cref):
    rng = random.Random(8)
    A, B = [], []
    for _ in range(1500):
        a, b = _edit(rng, "abcü", 0, 12)
        A.append(a)
        B.append(b)
    np_d = R.batch_numpy_distance(A, B)
    np_s = R.batch_numpy(A, B)
    for a, b, d, s in zip(A, B, np_d, np_s):
        assert R.distance(a, b) == R.distance(b, a) == cref.distance(a, b) == d
        assert R.score(a, b) == s
    md = R.mixed_distances(A + ["x" * 40 + "y"], B + ["y" + "x" * 40], cref)
    assert md[:-1].tolist() == np_d.tolist() and md[-1] == 2


def test_c_reference_on_long_strings_matches_python(cref):
    rng = random.Random(9)
    for _ in range(5):
        a, b = _edit(rng, "xyz", 150, 300)
        assert cref.lcs(a, b) == R.lcs(a, b)


def _widths(lp):
    return [W for W in (1, 2, 3, 4) if lp <= 32 * W]


@pytest.mark.parametrize("alphabet", ["ab", "abcdefgh"])
def test_lane_recurrence_every_length_pair(lane, cref, alphabet):
    """Pattern 0..128 x text 0..128 bytes under every W that holds the pattern (the carry crosses bits 32 / 64 / 96), columns run
    beyond the text as in a wave, and the unmasked (literal) form with tmax == lt."""
    rng = random.Random(128 + len(alphabet))
    for lp in range(129):
        for lt in range(129):
            p = "".join(rng.choice(alphabet) for _ in range(lp))
            t = list(p[:lt]) + [rng.choice(alphabet) for _ in range(lt - min(lp, lt))]
            for _ in range(rng.randint(0, 4)):
                if t:
                    t[rng.randrange(len(t))] = rng.choice(alphabet)
            t = "".join(t)
            want = cref.lcs(p, t)
            tmax = min(128, lt + rng.randint(0, 8))
            for W in _widths(lp):
                assert lane.indel_lane_lcs_w(p.encode(), lp, t.encode(), lt, tmax, W, 1) == want, (p, t, W)
            assert lane.indel_lane_lcs_w(p.encode(), lp, t.encode(), lt, lt, _widths(lp)[0], 0) == want, (p, t)


def test_lane_recurrence_random_pairs_and_nul_bytes(lane, cref):
    """Full ASCII including NUL (a NUL of the pattern must not match the zero padding behind a shorter text)."""
    rng = random.Random(129)
    alphabet = [chr(c) for c in range(0, 128)]
    for _ in range(3000):
        a, b = _edit(rng, rng.choice(["ab", "\0a", "etaoinshrdlu", alphabet]), 0, 128)
        a, b = a[:128], b[:128]
        p, t = (a, b) if len(a) >= len(b) else (b, a)
        want = cref.lcs(a, b)
        tmax = min(128, len(t) + rng.randint(0, 70))
        for W in _widths(len(p)):
            assert lane.indel_lane_lcs_w(p.encode(), len(p), t.encode(), len(t), tmax, W, 1) == want, (a, b, W)
        d = len(a) + len(b) - 2 * want
        assert lane.indel_score(d, len(a), len(b)) == R.normalise(d, len(a), len(b))


def test_lane_recurrence_known_answers(lane):
    for a, b, l, _ in R.KNOWN:
        if all(ord(c) < 128 for c in a + b):
            for p, t in ((a, b), (b, a)):
                for W in _widths(len(p)):
                    assert lane.indel_lane_lcs_w(p.encode(), len(p), t.encode(), len(t), len(t), W, 1) == l


def _u32(s):
    return np.array([ord(c) for c in s] or [0], dtype=np.uint32)


def test_wave_word_step_across_word_boundaries(lane, cref):
    """The 64-bit word step of k_indel_wave (carry of the add only) on lengths crossing 63/64/65, 127/128/129, 255/256/257."""
    rng = random.Random(256)
    lens = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300]
    for m in lens:
        for n in lens:
            for alphabet in ("ab", "abcdü\U0001F600"):
                p = "".join(rng.choice(alphabet) for _ in range(m))
                t = list(p[:n]) + [rng.choice(alphabet) for _ in range(n - min(m, n))]
                for _ in range(rng.randint(0, 6)):
                    if t:
                        t[rng.randrange(len(t))] = rng.choice(alphabet)
                t = "".join(t)
                want = cref.lcs(p, t)
                x, y = _u32(p), _u32(t)
                words = max(1, (m + 63) // 64)
                for w in {words, 4 if words == 3 else words, words + 1}:
                    assert lane.indel_words_lcs(x.ctypes.data, m, y.ctypes.data, n, w) == want, (m, n, w)


def test_epilogue_clamp_and_length_cut(lane):
    for s in range(0, 300):
        for l in range(0, s // 2 + 1, 7):
            assert lane.indel_score(s - 2 * l, s - l, l) == R.normalise(s - 2 * l, s - l, l)
    assert lane.indel_score(0, 0, 0) == 1.0
    for d in (0, 1, 3, 4, 17, 1000):
        for k in (0, 1, 3, 16, U):
            assert lane.indel_clamp(d, k) == R.clamp(d, k)
    assert lane.indel_length_cut(3, 7, 3) == 1 and lane.indel_length_cut(3, 7, 4) == 0 and lane.indel_length_cut(200, 0, U) == 0


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_measure_supported.argtypes = [C.c_int, C.c_int]
    L.strsim_last_error_message.restype = C.c_char_p
    L.strsim_abi_version.restype = C.c_uint32
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name in ("strsim_distance_device", "strsim_distance_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, vp, u64]
    return L


PAIRWISE, BEST_MATCH, CODEC = 0, 1, 2


def test_measure_supported(L):
    assert L.strsim_measure_supported(INDEL, PAIRWISE) == 1
    assert L.strsim_measure_supported(INDEL, BEST_MATCH) == 0
    assert L.strsim_measure_supported(INDEL, CODEC) == 0
    assert L.strsim_measure_supported(INDEL, 3) == 0
    for m in (5, 7, 9):
        for e in (PAIRWISE, BEST_MATCH, CODEC):
            assert L.strsim_measure_supported(m, e) == 0, (m, e)
    assert L.strsim_abi_version() == 0x00010007


@pytest.mark.parametrize("entry", ["strsim_distance_device", "strsim_distance_host"])
def test_distance_argument_errors_without_a_device(L, entry):
    f = getattr(L, entry)
    off = np.array([0, 1, 2], dtype=np.uint32)
    val = np.frombuffer(b"ab", dtype=np.uint8).copy()
    out = np.zeros(2, dtype=np.uint32)
    o, v, p = off.ctypes.data, val.ctypes.data, out.ctypes.data
    assert f(None, INDEL, o, v, 2, o, v, 3, U, p, 2) == 1  # shape
    assert L.strsim_last_error_message() == b"Inputs must have the same length, or one of them must be a Utf8 literal."
    assert f(None, INDEL, o, v, 2, o, v, 2, U, p, 3) == 2  # out_rows
    assert b"out_rows" in L.strsim_last_error_message()
    for args in ((None, v, o, v), (o, None, o, v), (o, v, None, v), (o, v, o, None)):
        assert f(None, INDEL, args[0], args[1], 2, args[2], args[3], 2, 1, p, 2) == 2
        assert b"NULL buffer" in L.strsim_last_error_message()
    assert f(None, INDEL, o, v, 2, o, v, 2, 1, None, 2) == 2
    assert f(None, INDEL, o, v, 2, o, v, 2, 1, p, 2) == 2  # every argument right: the NULL context
    assert b"ctx is NULL" in L.strsim_last_error_message()
    assert f(None, INDEL, o, v, 1, o, v, 2, 1, p, 2) == 2  # a literal on the left: shape ok, then the context
    assert b"ctx is NULL" in L.strsim_last_error_message()
    for m in (5, 7, 9):  # still no distance, and the text names the three that have one
        assert f(None, m, o, v, 2, o, v, 2, 3, p, 2) == 2
        msg = L.strsim_last_error_message()
        assert b"measure" in msg and b"STRSIM_LEVENSHTEIN" in msg and b"STRSIM_OSA" in msg and b"STRSIM_INDEL" in msg


def test_other_entry_points_refuse_indel_before_any_device(L):
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.strsim_pairs_device.restype = C.c_int
    L.strsim_pairs_device.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, vp, u64]
    L.strsim_best_match_host.restype = C.c_int
    L.strsim_best_match_host.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, C.c_double, vp, vp]
    L.strsim_nearest_host.restype = C.c_int
    L.strsim_nearest_host.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, u32, vp, vp]
    L.strsim_codec_create.restype = C.c_int
    assert L.strsim_pairs_device(None, INDEL, None, None, 1, None, None, 1, None, 1) == 2
    assert b"ctx is NULL" in L.strsim_last_error_message()  # (the measure itself is accepted)
    assert L.strsim_best_match_host(None, INDEL, None, None, 0, None, None, 0, 1, 0.0, None, None) == 2
    assert b"measure" in L.strsim_last_error_message()
    assert L.strsim_nearest_host(None, INDEL, None, None, 0, None, None, 0, 1, 1, None, None) == 2
    assert b"measure" in L.strsim_last_error_message()


def test_python_surface_without_a_device(L):
    import strsim_amd as S
    assert S.MEASURE_ID["indel"] == INDEL and S.INDEL_MEASURES == ("indel",)
    assert S.MEASURES == ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")
    assert S.EXTRA_MEASURES == ("osa",) and S.DISTANCE_MEASURES == ("levenshtein", "osa")
    assert S.measure_supported("indel") and not S.measure_supported("indel", "best_match") and not S.measure_supported("indel", "codec")
    for name in ("indel", "indel_distance", "INDEL_MEASURES"):
        assert name in S.__all__ and hasattr(S, name)
    with pytest.raises(ValueError, match="no distance"):
        S.nearest("indel", ["a"], ["b"])
    with pytest.raises(ValueError, match="no best match"):
        S.best_match("indel", ["a"], ["b"])
    with pytest.raises(ValueError, match="no distance"):
        S.distance("jaro", ["a"], ["b"])


def test_polars_wrapper_source_lists_indel():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert re.search(r'__all__ = \[[^\]]*"indel_distance"[^\]]*"indel"', src)
    assert "fuzz.ratio" in src and "substitution costs 2" in src


def test_field_functions():
    pa = pytest.importorskip("pyarrow")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    from strsim_amd import arrow_host
    assert arrow_host.field_plugin("indel", ("left", "right")) == ("left", pa.float64())
    assert arrow_host.field_plugin("indel_distance", ("left", "right")) == ("left", pa.uint32())
    assert arrow_host.field_plugin("indel_distance", ("q", "c", "max_distance")) == ("q", pa.uint32())


def test_header_declares_and_library_exports_the_plugin_symbols(L):
    hdr = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    assert "POLARS_PLUGIN_DECLARE(indel)" in hdr and "POLARS_PLUGIN_DECLARE(indel_distance)" in hdr
    assert re.search(r"STRSIM_INDEL\s*=\s*8\b", open(os.path.join(ROOT, "include", "strsim_amd.h")).read())
    for sym in ("_polars_plugin_indel", "_polars_plugin_indel_distance", "_polars_plugin_field_indel", "_polars_plugin_field_indel_distance"):
        assert hasattr(L, sym), sym
