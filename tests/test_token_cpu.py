"""token_sort_ratio / token_set_ratio (measure ids 14 and 16) without a GPU: the model (tests/token_ref.py) against known answers
and against its own brute force, the whitespace set against str.isspace, the g++ build of the device cores of strsim_token.h
against the model, and the C ABI / Python surfaces as far as they go without a device."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import token_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "token_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
SORT, SET = 14, 16
PAIRWISE, BEST_MATCH, CODEC = 0, 1, 2


# ---- the model ----

def test_known_answers():
    # rapidfuzz's documentation
    assert R.token_sort_ratio("fuzzy wuzzy was a bear", "wuzzy fuzzy was a bear") == 1.0
    assert R.token_set_ratio("fuzzy was a bear", "fuzzy fuzzy was a bear") == 1.0
    # the issue's pair: both sides normalise to "john smith"
    assert R.token_sort("smith john") == R.token_sort("john  smith") == "john smith"
    assert R.token_sort_ratio("smith john", "john  smith") == 1.0
    # by hand.  "b a" -> "a b", "a c" -> "a c": LCS("a b", "a c") = "a " = 2, d = 3 + 3 - 4 = 2, 1 - 2/6
    assert R.token_sort_ratio("b a", "a c") == 1.0 - 2.0 / 6.0
    # duplicates are kept by the sort form: "a a" against "a": LCS 1, d = 3 + 1 - 2 = 2, 1 - 2/4
    assert R.token_sort_ratio("a a", "a") == 0.5
    # ... and dropped by the set form: {a} and {a}: the intersection is not empty and both differences are -> 1.0
    assert R.token_set_ratio("a a", "a") == 1.0
    # no tokens: the sort form falls out of indel ("" against "": 1.0; "" against "a": d = 1, 1 - 1/1 = 0.0); the set form is 0.0
    assert R.token_sort_ratio(" \t", "") == 1.0 and R.token_sort_ratio("  ", "a") == 0.0
    assert R.token_set_ratio(" ", "") == 0.0 and R.token_set_ratio("", "a") == 0.0
    # set form, disjoint sets {ab} / {cd}: sl = 0, r0 = indel("ab", "cd") = 1 - 4/4 = 0.0
    assert R.token_set_ratio("ab", "cd") == 0.0
    # set form with all three parts: A = {x, ab}, B = {x, ac}: sect = "x" (sl 1), ab = "ab", ba = "ac" (la = lb = 2), sep = 1,
    # sab = sba = 4; d = indel_distance("ab", "ac") = 2 -> r0 = 1 - 2/8 = 0.75; E(1 + 2, 1 + 4) = 1 - 3/5 = 0.4 twice; max = 0.75
    assert R.token_set_ratio("x ab", "ac x") == 0.75
    # set form where the intersection wins: A = {x, y, z, a}, B = {x, y, z, b}: sect = "x y z" (sl 5), la = lb = 1, sab = sba = 7;
    # d = 2 -> r0 = 1 - 2/14; E(2, 12) = 1 - 2/12 is lower, so r0 = 0.857142...
    assert R.token_set_ratio("x y z a", "b z y x") == 1.0 - 2.0 / 14.0
    # a token that is a prefix of another sorts first; NUL is a token character and sorts before everything
    assert R.token_sort("ab a abc \0") == "\0 a ab abc"
    # U+00A0 and U+3000 split, U+200B (zero width space, not in str.isspace) does not
    assert R.token_sort("b\u00a0a\u3000c") == "a b c" and R.token_sort("b\u200ba") == "b\u200ba"


def test_whitespace_set_is_str_isspace():
    assert len(R.WHITESPACE) == 29 and len(set(R.WHITESPACE)) == 29
    assert sorted(R.WHITESPACE) == [c for c in range(0x110000) if chr(c).isspace()]
    # ... and it is what str.split() splits at
    for c in R.WHITESPACE:
        assert ("a" + chr(c) + "b").split() == ["a", "b"], hex(c)


# every whitespace code point, NUL, ASCII, Cyrillic, CJK, a four-byte character, and near misses of the whitespace encodings:
# U+200B, U+1681, U+2027 and U+00C2 share bytes with U+200A, U+1680, U+2028 and the lead byte of U+0085
ALPHABET = [chr(c) for c in R.WHITESPACE] + ["\0", "a", "b", "c", "ab", "\u0436", "\u044f", "\u6f22", "\u5b57", "\U0001F600",
                                             "\u200b", "\u1681", "\u2027", "\u00c2"]


def _random_string(rng, n=14):
    return "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, n)))


def test_set_rule_equals_the_three_string_brute_force():
    rng = random.Random(11)
    A, B = R.gen_frame(5, 3000)
    pairs = list(zip(A, B)) + [(_random_string(rng), _random_string(rng)) for _ in range(3000)]
    pairs += [("", ""), (" ", ""), ("", "\t\n"), ("a", ""), ("", "a"), ("a", " "), ("a b", "a"), ("a", "a b"), ("a b", "b a")]
    small = ["".join(t) for k in range(5) for t in itertools.product("ab ", repeat=k)]
    pairs += [(x, y) for x in small for y in small]
    for a, b in pairs:
        assert R.set_rule(a, b) == R.token_set_brute(a, b), (a, b)


def test_frame_helpers_equal_the_row_functions():
    A, B = R.gen_frame(3, 400)
    s1, s2 = R.frame_sort_ratio(A, B), R.frame_set_ratio(A, B)
    for i in range(len(A)):
        assert s1[i] == R.token_sort_ratio(A[i], B[i]) and s2[i] == R.set_rule(A[i], B[i])


def test_generator_share_of_trivial_scores():
    """The random frames of the GPU tests must not be mostly 0.0 / 1.0: at most 30 % (on the model's output)."""
    A, B = R.gen_frame(1, 20000)
    for s in (R.frame_sort_ratio(A, B), R.frame_set_ratio(A, B)):
        assert float(((s == 0.0) | (s == 1.0)).mean()) <= 0.30


# ---- the g++ build of the device cores ----

@pytest.fixture(scope="module")
def cores():
    d = tempfile.mkdtemp(prefix="token_harness_")
    so = os.path.join(d, "token_harness.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    L.token_sort_c.restype = C.c_uint32
    L.token_sort_c.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_int]
    L.token_set_c.restype = None
    L.token_set_c.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int]
    L.token_set_score_c.restype = C.c_double
    L.token_set_score_c.argtypes = [C.c_uint32] * 5
    L.token_space_len_c.restype = C.c_uint32
    L.token_space_len_c.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32]
    return L


def _c_sort(L, s, lane):
    b = s.encode("utf-8")
    out = C.create_string_buffer(len(b) + 1)
    n = L.token_sort_c(b, len(b), out, lane)
    assert n <= len(b)
    return out.raw[:n].decode("utf-8")


def _c_set(L, a, b, lane):
    xa, xb = a.encode("utf-8"), b.encode("utf-8")
    oa, ob = C.create_string_buffer(len(xa) + 1), C.create_string_buffer(len(xb) + 1)
    res = (C.c_uint32 * 6)()
    L.token_set_c(xa, len(xa), xb, len(xb), oa, ob, res, lane)
    assert res[4] <= len(xa) and res[5] <= len(xb)
    return oa.raw[:res[4]].decode("utf-8"), ob.raw[:res[5]].decode("utf-8"), tuple(res[:4])


def _check_pair(L, a, b, lane):
    ab, ba, (sl, la, lb, flags) = _c_set(L, a, b, lane)
    sect, eab, eba = R.set_parts(a, b)
    assert (ab, ba) == (eab, eba), (a, b, lane)
    assert (sl, la, lb) == (len(sect), len(eab), len(eba)), (a, b, lane)
    assert L.token_set_score_c(sl, la, lb, flags, R.indel_distance(eab, eba)) == R.set_rule(a, b), (a, b, lane)


def test_cores_whitespace_bytes(cores):
    for c in range(0x110000):
        if 0xD800 <= c < 0xE000:
            continue
        b = chr(c).encode("utf-8")
        want = len(b) if chr(c).isspace() else 0
        if cores.token_space_len_c(b, 0, len(b)) != want:
            raise AssertionError(hex(c))


@pytest.mark.parametrize("lane", [1, 0])
def test_cores_exhaustive_short_strings(cores, lane):
    strings = ["".join(t) for k in range(9) for t in itertools.product("ab ", repeat=k)]
    for s in strings:
        assert _c_sort(cores, s, lane) == R.token_sort(s), (s, lane)
    short = [s for s in strings if len(s) <= 5]
    for a in short:
        for b in short[::3]:
            _check_pair(cores, a, b, lane)


@pytest.mark.parametrize("lane", [1, 0])
def test_cores_random_unicode_strings(cores, lane):
    rng = random.Random(7 + lane)
    for _ in range(6000):
        a, b = _random_string(rng), _random_string(rng)
        assert _c_sort(cores, a, lane) == R.token_sort(a), (a, lane)
        _check_pair(cores, a, b, lane)


def test_cores_many_tokens(cores):
    """The sorting network at sizes that are not powers of two, and the 1 000 one-letter tokens of the issue."""
    rng = random.Random(3)
    letters = "abcdefghijklmnopqrstuvwxyz"
    thousand = " ".join(rng.choice(letters) for _ in range(1000))
    for lane in (0, 1):
        assert _c_sort(cores, thousand, lane) == R.token_sort(thousand)
    for n in list(range(1, 70)) + [127, 128, 129, 300, 513]:
        s = "  ".join("".join(rng.choice("abc") for _ in range(rng.randint(1, 4))) for _ in range(n))
        t = " ".join("".join(rng.choice("abc") for _ in range(rng.randint(1, 4))) for _ in range(n // 2 + 1))
        assert _c_sort(cores, s, 0) == R.token_sort(s), n
        ab, ba, _ = _c_set(cores, s, t, 0)
        assert (ab, ba) == R.set_parts(s, t)[1:], n


# ---- the C ABI without a device ----

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
    for name in ("strsim_token_sort_device", "strsim_token_sort_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64]
    for name in ("strsim_pairs_device", "strsim_pairs_device_small", "strsim_pairs_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, vp, u64]
    for name in ("strsim_distance_device", "strsim_distance_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, vp, u64]
    for name in ("strsim_partial_alignment_device", "strsim_partial_alignment_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, u64]
    for name in ("strsim_best_match_device", "strsim_best_match_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, C.c_double, vp, vp]
    for name in ("strsim_nearest_device", "strsim_nearest_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, u32, vp, vp]
    L.strsim_codec_create.restype = C.c_int
    L.strsim_codec_create.argtypes = [vp, C.c_int, u32, vp]
    L.strsim_ctx_last_token_wave_rows.restype = u64
    L.strsim_ctx_last_token_wave_rows.argtypes = [vp]
    return L


def test_token_measure_supported_and_abi_version(L):
    for m in (SORT, SET):
        assert L.strsim_measure_supported(m, PAIRWISE) == 1
        assert L.strsim_measure_supported(m, BEST_MATCH) == 0
        assert L.strsim_measure_supported(m, CODEC) == 0
        assert L.strsim_measure_supported(m, 3) == 0
    for m in (5, 7, 9, 11, 12, 13, 15, 17, 100, -1):
        for e in (PAIRWISE, BEST_MATCH, CODEC):
            assert L.strsim_measure_supported(m, e) == 0, (m, e)
    assert L.strsim_abi_version() == 0x00010007
    assert L.strsim_ctx_last_token_wave_rows(None) == 0


@pytest.mark.parametrize("measure", [SORT, SET])
def test_pairwise_argument_errors_without_a_device(L, measure):
    off = np.array([0, 1, 2], dtype=np.uint32)
    val = np.frombuffer(b"ab", dtype=np.uint8).copy()
    out = np.zeros(2, dtype=np.float64)
    o, v, r = off.ctypes.data, val.ctypes.data, out.ctypes.data
    for name in ("strsim_pairs_device", "strsim_pairs_device_small", "strsim_pairs_host"):
        f = getattr(L, name)
        assert f(None, measure, o, v, 2, o, v, 2, r, 2) == 2
        assert b"ctx is NULL" in L.strsim_last_error_message()  # (the measure itself is accepted)
    # behind the context check the entry points look at the shape before they touch a device (the stand-in is never dereferenced)
    ctx_stand_in = C.create_string_buffer(8)
    for name in ("strsim_pairs_device", "strsim_pairs_device_small"):
        f = getattr(L, name)
        assert f(ctx_stand_in, measure, o, v, 2, o, v, 3, r, 2) == 1
        assert L.strsim_last_error_message() == b"Inputs must have the same length, or one of them must be a Utf8 literal."
        assert f(ctx_stand_in, measure, o, v, 2, o, v, 2, r, 3) == 2
        assert b"out_rows" in L.strsim_last_error_message()
        assert f(ctx_stand_in, measure, None, v, 2, o, v, 2, r, 2) == 2
        assert b"NULL buffer" in L.strsim_last_error_message()
        assert f(ctx_stand_in, measure, o, v, 2, o, v, 2, None, 2) == 2
        assert b"NULL" in L.strsim_last_error_message()
        for m in (13, 15, 17):
            assert f(ctx_stand_in, m, o, v, 2, o, v, 2, r, 2) == 2
            assert b"unknown measure" in L.strsim_last_error_message()


@pytest.mark.parametrize("entry", ["strsim_token_sort_device", "strsim_token_sort_host"])
def test_token_sort_argument_errors_without_a_device(L, entry):
    f = getattr(L, entry)
    off = np.array([0, 1, 2], dtype=np.uint32)
    val = np.frombuffer(b"ab", dtype=np.uint8).copy()
    out_off = np.zeros(3, dtype=np.uint32)
    out_val = np.zeros(2, dtype=np.uint8)
    o, v, oo, ov = off.ctypes.data, val.ctypes.data, out_off.ctypes.data, out_val.ctypes.data
    assert f(None, o, v, 1 << 32, oo, ov, 2) == 2
    assert b"rows in one call" in L.strsim_last_error_message()
    for args in ((None, v, oo, ov), (o, None, oo, ov), (o, v, None, ov), (o, v, oo, None)):
        assert f(None, args[0], args[1], 2, args[2], args[3], 2) == 2
        assert b"NULL buffer" in L.strsim_last_error_message()
    assert f(None, o, v, 2, oo, ov, 2) == 2  # every argument right: the NULL context
    assert b"ctx is NULL" in L.strsim_last_error_message()
    assert f(None, o, None, 0, oo, None, 0) == 2  # zero rows: the offsets and the context are all there is to check
    assert b"ctx is NULL" in L.strsim_last_error_message()
    if entry == "strsim_token_sort_host":  # the host variant knows the column's size without a device
        ctx_stand_in = C.create_string_buffer(8)
        assert f(ctx_stand_in, o, v, 2, oo, ov, 1) == 2
        assert b"out_capacity=1 but the column holds 2 bytes" in L.strsim_last_error_message()


def test_other_entry_points_refuse_the_token_measures_before_any_device(L):
    for m in (SORT, SET):
        for name in ("strsim_best_match_device", "strsim_best_match_host"):
            assert getattr(L, name)(None, m, None, None, 0, None, None, 0, 1, 0.0, None, None) == 2
            assert b"unknown measure %d" % m in L.strsim_last_error_message()
        for name in ("strsim_nearest_device", "strsim_nearest_host"):
            assert getattr(L, name)(None, m, None, None, 0, None, None, 0, 1, 1, None, None) == 2
            assert b"measure %d has no distance (STRSIM_LEVENSHTEIN or STRSIM_OSA)" % m in L.strsim_last_error_message()
        for name in ("strsim_distance_device", "strsim_distance_host"):
            assert getattr(L, name)(None, m, None, None, 0, None, None, 0, 1, None, 0) == 2
            msg = L.strsim_last_error_message()
            assert b"measure %d has no distance" % m in msg and b"STRSIM_INDEL" in msg
        out = C.c_void_p()
        ctx_stand_in = C.create_string_buffer(8)  # (never dereferenced: the measure is refused first)
        assert L.strsim_codec_create(ctx_stand_in, m, 32, C.byref(out)) == 2
        assert b"bad measure" in L.strsim_last_error_message() and not out.value


# ---- the Python surfaces ----

def test_token_python_surface_without_a_device(L):
    import strsim_amd as S
    assert S.TOKEN_MEASURES == ("token_sort_ratio", "token_set_ratio")
    assert S.MEASURE_ID["token_sort_ratio"] == SORT and S.MEASURE_ID["token_set_ratio"] == SET
    assert S.MEASURES == ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")
    assert S.EXTRA_MEASURES == ("osa",) and S.DISTANCE_MEASURES == ("levenshtein", "osa") and S.INDEL_MEASURES == ("indel",)
    assert S.PARTIAL_MEASURES == ("partial_ratio",)
    for m in S.TOKEN_MEASURES:
        assert S.measure_supported(m) and not S.measure_supported(m, "best_match") and not S.measure_supported(m, "codec")
        with pytest.raises(ValueError, match="no distance"):
            S.distance(m, ["a"], ["b"])
        with pytest.raises(ValueError, match="no distance"):
            S.nearest(m, ["a"], ["b"])
        with pytest.raises(ValueError, match="no best match"):
            S.best_match(m, ["a"], ["b"])
    for name in ("token_sort_ratio", "token_set_ratio", "token_sort", "TOKEN_MEASURES"):
        assert name in S.__all__ and hasattr(S, name)
    for name in ("token_sort_host", "token_sort_device", "last_token_wave_rows"):
        assert hasattr(S.Context, name)


def test_polars_wrapper_source_lists_the_token_ratios():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert re.search(r'__all__ = \[[^\]]*"partial_ratio_alignment"[^\]]*"token_sort_ratio"[^\]]*"token_set_ratio"', src)
    for fn in ("token_sort_ratio", "token_set_ratio"):
        doc = re.search(r'def %s\(expr: IntoExpr, other: IntoExpr\) -> pl\.Expr:\n    """(.*?)"""' % fn, src, re.S).group(1)
        assert "fuzz." + fn in doc and "/ 100" in doc and "str.isspace" in doc and "upstream polars-strsim" in doc


def test_headers_declare_and_library_exports_the_token_symbols(L):
    hdr = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    assert "POLARS_PLUGIN_DECLARE(token_sort_ratio)" in hdr and "POLARS_PLUGIN_DECLARE(token_set_ratio)" in hdr
    api = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    assert re.search(r"STRSIM_TOKEN_SORT_RATIO\s*=\s*14\b", api) and re.search(r"STRSIM_TOKEN_SET_RATIO\s*=\s*16\b", api)
    assert re.search(r"#define STRSIM_ABI_VERSION 0x00010007u", api)
    for sym in ("_polars_plugin_token_sort_ratio", "_polars_plugin_token_set_ratio", "_polars_plugin_field_token_sort_ratio",
                "_polars_plugin_field_token_set_ratio", "strsim_token_sort_device", "strsim_token_sort_host",
                "strsim_ctx_last_token_wave_rows"):
        assert hasattr(L, sym), sym
        assert sym in api or sym.startswith("_polars_plugin")


def test_token_field_functions():
    pa = pytest.importorskip("pyarrow")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    from strsim_amd import arrow_host
    for fn in ("token_sort_ratio", "token_set_ratio"):
        assert arrow_host.field_plugin(fn, ("left", "right")) == ("left", pa.float64())
