"""token_ratio, the partial token ratios and wratio (ids 18 .. 26) without a GPU: the model (tests/wratio_ref.py) against known
answers and against a transcription of rapidfuzz's early-exit form, the g++ build of the cores of strsim_wratio.h (class predicate,
combine rule, the rule of partial_token_set_ratio, the row copy of the gather) against the model, and the C ABI / Python surfaces
as far as they go without a device."""
import ctypes as C
import os
import random
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import partial_ref
import token_ref as T
import wratio_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "wratio_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
IDS = (18, 20, 22, 24, 26)
NAMES = ("token_ratio", "partial_token_sort_ratio", "partial_token_set_ratio", "partial_token_ratio", "wratio")
PAIRWISE, BEST_MATCH, CODEC = 0, 1, 2


def bits(x):
    return struct.pack("<d", float(x))


# ---- the model ----

def test_wratio_model_worked_example_of_the_rapidfuzz_documentation():
    a, b = "this is a test", "this is a new test!!!"
    assert (len(a), len(b)) == (14, 21) and W.wratio_class(14, 21) == W.FAR8  # 2 * 21 == 3 * 14: not near
    assert bits(T.indel(a, b)) == bits(1.0 - 7.0 / 35.0)  # r = 28 / 35
    assert W.partial_token_ratio(a, b) == 1.0  # a common token
    assert bits(W.wratio(a, b)) == bits((1.0 * 0.95) * 0.9)
    assert round(100 * W.wratio(a, b), 6) == 85.5


def test_wratio_model_known_answers():
    a, b = "fuzzy wuzzy was a bear", "wuzzy fuzzy was a bear"
    assert W.token_ratio(a, b) == 1.0 and W.partial_token_sort_ratio(a, b) == 1.0
    assert W.partial_token_set_ratio(a, b) == 1.0 and W.partial_token_ratio(a, b) == 1.0
    assert bits(W.wratio(a, b)) == bits(max(T.indel(a, b), 1.0 * 0.95))
    # duplicate tokens: the sort form keeps them, the set form does not
    a, b = "ab ab", "abab"
    assert bits(W.partial_token_sort_ratio(a, b)) == bits(0.75) and W.partial_token_set_ratio(a, b) == 1.0
    assert W.partial_token_ratio(a, b) == 1.0 and W.partial_token_ratio_rapidfuzz(a, b) == 1.0
    # no common token, no duplicates: both partial scores are the same string pair
    a, b = "new york mets", "yankees atlanta"
    assert bits(W.partial_token_sort_ratio(a, b)) == bits(W.partial_token_set_ratio(a, b))
    # near and far > 8
    assert bits(W.wratio("abcd", "abce")) == bits(max(0.75, W.token_ratio("abcd", "abce") * 0.95)) == bits(0.75)
    a, b = "ab", "xx ab xxxxxxxxxxxxxx"
    assert W.wratio_class(len(a), len(b)) == W.FAR
    assert bits(W.wratio(a, b)) == bits(max(T.indel(a, b), 1.0 * 0.6, (1.0 * 0.95) * 0.6)) == bits(0.6)


def test_wratio_model_empty_and_whitespace_only_strings():
    # (a, b) -> token_ratio, partial_token_sort_ratio, partial_token_set_ratio, partial_token_ratio, wratio
    want = {
        ("", ""): (1.0, 1.0, 0.0, 1.0, 0.0),
        ("", "abc"): (0.0, 0.0, 0.0, 0.0, 0.0),
        ("abc", ""): (0.0, 0.0, 0.0, 0.0, 0.0),
        (" ", "\t"): (1.0, 1.0, 0.0, 1.0, 0.95),          # near; r = 0, both token-sorted strings are empty
        ("  ", "x"): (0.0, 0.0, 0.0, 0.0, 0.0),           # far; every sub-score is 0
        ("　 ", " "): (1.0, 1.0, 0.0, 1.0, (1.0 * 0.95) * 0.9),  # far <= 8: partial_ratio is 0, partial_token_ratio 1
        (" x ", "x"): (1.0, 1.0, 1.0, 1.0, 1.0 * 0.9),            # far: partial_ratio = 1 beats (1 * 0.95) * 0.9 and r = 0.5
    }
    for (a, b), exp in want.items():
        got = tuple(W.SCORE[n](a, b) for n in NAMES)
        assert [bits(g) for g in got] == [bits(e) for e in exp], (a, b, got, exp)


def test_wratio_model_class_boundaries():
    for la, lb, cls in ((2, 3, W.FAR8), (4, 6, W.FAR8), (5, 7, W.NEAR), (3, 4, W.NEAR), (1, 8, W.FAR8), (4, 32, W.FAR8), (1, 9, W.FAR),
                        (4, 33, W.FAR), (0, 0, W.EMPTY), (0, 5, W.EMPTY), (1, 1, W.NEAR), (2, 2, W.NEAR)):
        assert W.wratio_class(la, lb) == cls == W.wratio_class(lb, la), (la, lb)
    assert W.wratio_class(len("éé"), len("abc")) == W.FAR8 and W.wratio_class(len("éé".encode()), len("abc")) == W.NEAR


def test_partial_token_ratio_is_the_early_exit_form_of_rapidfuzz():
    """max(partial_token_sort_ratio, partial_token_set_ratio) against the transcription, 4 000 rows of one to four tokens over a
    vocabulary of three (duplicates in most rows).  The partial ratios are the C brute force of partial_ref, batched."""
    rng = random.Random(1826)
    vocab_a, vocab_b = ("ab", "abc", "b"), ("ab", "ba", "cab", "abc", "b")
    rows = []
    for i in range(4000):
        va = vocab_a
        vb = vocab_a if i % 4 == 0 else vocab_b[1:4]  # three tokens each: a quarter of the rows can share tokens
        rows.append((" ".join(rng.choice(va) for _ in range(rng.randint(1, 4))), " ".join(rng.choice(vb) for _ in range(rng.randint(1, 4)))))
    asked = []

    def record(x, y):
        asked.append((x, y))
        return 0.0

    for a, b in rows:
        W.partial_token_ratio(a, b, record)
        W.partial_token_ratio_rapidfuzz(a, b, record)
    pairs = sorted(set(asked))
    scores = partial_ref.CRef().batch([p[0] for p in pairs], [p[1] for p in pairs])[0]
    table = {p: float(s) for p, s in zip(pairs, scores)}
    lookup = lambda x, y: table[(x, y)]
    differ = shared = 0
    for a, b in rows:
        assert bits(W.partial_token_ratio(a, b, lookup)) == bits(W.partial_token_ratio_rapidfuzz(a, b, lookup)), (a, b)
        differ += W.partial_token_sort_ratio(a, b, lookup) != W.partial_token_set_ratio(a, b, lookup)
        shared += bool(set(a.split()) & set(b.split()))
    assert differ > 500 and 300 < shared < 3500  # the frame does exercise both branches
    for a, b in rows[:40]:  # the batched brute force is the Python one
        assert bits(lookup(T.token_sort(a), T.token_sort(b))) == bits(W.partial_ratio(T.token_sort(a), T.token_sort(b)))


# ---- the g++ build of the cores ----

@pytest.fixture(scope="module")
def cores():
    d = tempfile.mkdtemp(prefix="wratio_harness_")
    so = os.path.join(d, "wratio_harness.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    L.wratio_class_c.restype = C.c_uint32
    L.wratio_class_c.argtypes = [C.c_uint32, C.c_uint32]
    L.wratio_rule_c.restype = C.c_double
    L.wratio_rule_c.argtypes = [C.c_uint32, C.c_double, C.c_double, C.c_double]
    L.partial_token_set_score_c.restype = C.c_double
    L.partial_token_set_score_c.argtypes = [C.c_uint32] * 4 + [C.c_double]
    L.take_copy_c.restype = None
    L.take_copy_c.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    return L


def test_wratio_class_and_rule_cores_match_the_model_on_the_length_grid(cores):
    grid = [0.0, 1.0, 0.5, 1.0 / 3.0, 2.0 / 3.0, 0.8, 28.0 / 35.0, 0.855, 0.95, 0.9, 0.6, 0.57, 0.1, 0.75]
    n = 0
    for la in range(41):
        for lb in range(41):
            cls = W.wratio_class(la, lb)
            assert cores.wratio_class_c(la, lb) == cls, (la, lb)
            for k, r in enumerate(grid):
                s0, s1 = grid[(k + la) % len(grid)], grid[(k + 2 * lb + 1) % len(grid)]
                assert bits(cores.wratio_rule_c(cls, r, s0, s1)) == bits(W.wratio_rule(cls, r, s0, s1)), (la, lb, r, s0, s1)
                n += 1
    assert n == 41 * 41 * len(grid)
    for cls in (W.EMPTY, W.NEAR, W.FAR8, W.FAR):  # every triple of the grid at every class
        for r in grid:
            for s0 in grid:
                for s1 in grid:
                    assert bits(cores.wratio_rule_c(cls, r, s0, s1)) == bits(W.wratio_rule(cls, r, s0, s1))
    assert cores.wratio_class_c(0xFFFFFFFF, 0xAAAAAAAB) == W.wratio_class(0xFFFFFFFF, 0xAAAAAAAB) == W.NEAR  # (no 32-bit overflow)
    assert cores.wratio_class_c(0xFFFFFFFF, 0x20000000) == W.wratio_class(0xFFFFFFFF, 0x20000000) == W.FAR8
    assert cores.wratio_class_c(0xFFFFFFFF, 0x1FFFFFFF) == W.FAR


def test_partial_token_set_score_core(cores):
    ZERO, ONE = 1, 2  # TOKEN_FLAG_*
    for p in (0.0, 0.25, 1.0):
        assert cores.partial_token_set_score_c(0, 3, 3, ZERO, p) == 0.0
        assert cores.partial_token_set_score_c(2, 0, 3, ONE, p) == 1.0    # a common token, one difference empty
        assert cores.partial_token_set_score_c(2, 3, 3, 0, p) == 1.0      # a common token, both differences there
        assert cores.partial_token_set_score_c(0, 3, 3, 0, p) == p


def test_take_copy_core_at_every_alignment(cores):
    """The row copy of the gather: every source and destination alignment, lengths 0 .. 40; nothing outside the row is written."""
    src = np.arange(1, 129, dtype=np.uint8)
    base = np.zeros(160, dtype=np.uint8)
    assert src.ctypes.data % 4 == 0 and base.ctypes.data % 4 == 0
    for sa in range(4):
        for da in range(4):
            for n in range(41):
                dst = base.copy()
                dst[:] = 0xEE
                cores.take_copy_c(src.ctypes.data + 4 + sa, dst.ctypes.data + 8 + da, n)
                exp = np.full(160, 0xEE, dtype=np.uint8)
                exp[8 + da:8 + da + n] = src[4 + sa:4 + sa + n]
                assert (dst == exp).all(), (sa, da, n)


# ---- the C ABI without a device ----

@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "library not built"
    L = C.CDLL(LIB)
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_measure_supported.argtypes = [C.c_int, C.c_int]
    L.strsim_last_error_message.restype = C.c_char_p
    L.strsim_abi_version.restype = C.c_uint32
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name in ("strsim_pairs_device", "strsim_pairs_device_small", "strsim_pairs_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, vp, u64]
    for name in ("strsim_distance_device", "strsim_distance_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, vp, u64]
    for name in ("strsim_best_match_device", "strsim_best_match_host", "strsim_extract_device", "strsim_extract_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, C.c_double, vp, vp]
    for name in ("strsim_nearest_device", "strsim_nearest_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, u32, vp, vp]
    L.strsim_codec_create.restype = C.c_int
    L.strsim_codec_create.argtypes = [vp, C.c_int, u32, vp]
    L.strsim_ctx_last_wratio_rows.restype = C.c_int
    L.strsim_ctx_last_wratio_rows.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    return L


def test_wratio_measure_supported_and_abi_version(L):
    for m in IDS:
        assert L.strsim_measure_supported(m, PAIRWISE) == 1
        assert L.strsim_measure_supported(m, BEST_MATCH) == 0
        assert L.strsim_measure_supported(m, CODEC) == 0
        assert L.strsim_measure_supported(m, 3) == 0
    for m in (5, 7, 9, 11, 12, 13, 15, 17, 19, 21, 23, 25, 27, 28):
        for e in (PAIRWISE, BEST_MATCH, CODEC):
            assert L.strsim_measure_supported(m, e) == 0, (m, e)
    assert L.strsim_abi_version() == 0x00010007
    near, far = C.c_uint64(7), C.c_uint64(7)
    assert L.strsim_ctx_last_wratio_rows(None, C.byref(near), C.byref(far)) == 2
    assert (near.value, far.value) == (0, 0) and b"ctx is NULL" in L.strsim_last_error_message()


@pytest.mark.parametrize("measure", IDS)
def test_wratio_pairwise_argument_errors_without_a_device(L, measure):
    off = np.array([0, 1, 2], dtype=np.uint32)
    val = np.frombuffer(b"ab", dtype=np.uint8).copy()
    out = np.zeros(2, dtype=np.float64)
    o, v, r = off.ctypes.data, val.ctypes.data, out.ctypes.data
    for name in ("strsim_pairs_device", "strsim_pairs_device_small", "strsim_pairs_host"):
        f = getattr(L, name)
        assert f(None, measure, o, v, 2, o, v, 2, r, 2) == 2
        assert b"ctx is NULL" in L.strsim_last_error_message()  # (the measure itself is accepted)
    ctx_stand_in = C.create_string_buffer(8)  # (never dereferenced: the shape is looked at before any device)
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
        for m in (measure - 1, measure + 1):
            assert f(ctx_stand_in, m, o, v, 2, o, v, 2, r, 2) == 2
            assert b"unknown measure" in L.strsim_last_error_message()


def test_other_entry_points_refuse_the_weighted_measures_before_any_device(L):
    for m in IDS:
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
        for name in ("strsim_extract_device", "strsim_extract_host"):
            assert getattr(L, name)(None, m, None, None, 0, None, None, 0, 1, 0.0, None, None) == 2
            assert b"scorer %d is not a scorer of extract" % m in L.strsim_last_error_message()
        out = C.c_void_p()
        ctx_stand_in = C.create_string_buffer(8)  # (never dereferenced: the measure is refused first)
        assert L.strsim_codec_create(ctx_stand_in, m, 32, C.byref(out)) == 2
        assert b"bad measure" in L.strsim_last_error_message() and not out.value


# ---- the Python surfaces ----

def test_wratio_python_surface_without_a_device(L):
    import strsim_amd as S
    assert S.WEIGHTED_MEASURES == NAMES
    assert [S.MEASURE_ID[n] for n in NAMES] == list(IDS) == [W.IDS[n] for n in NAMES]
    assert S.TOKEN_MEASURES == ("token_sort_ratio", "token_set_ratio") and S.PARTIAL_MEASURES == ("partial_ratio",)
    assert S.MEASURES == ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")
    assert S.EXTRACT_SCORERS == ("ratio", "token_sort_ratio")
    for m in NAMES:
        assert S.measure_supported(m) and not S.measure_supported(m, "best_match") and not S.measure_supported(m, "codec")
        with pytest.raises(ValueError, match="no distance"):
            S.distance(m, ["a"], ["b"])
        with pytest.raises(ValueError, match="no distance"):
            S.nearest(m, ["a"], ["b"])
        with pytest.raises(ValueError, match="no best match"):
            S.best_match(m, ["a"], ["b"])
        with pytest.raises(ValueError, match="no extract"):
            S.extract(m, ["a"], ["b"])
        assert m in S.__all__ and callable(getattr(S, m))
    assert "WEIGHTED_MEASURES" in S.__all__ and callable(S.Context.last_wratio_rows)


def test_polars_wrapper_source_lists_the_weighted_ratios():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    order = r'[^\]]*'.join('"%s"' % n for n in ("token_set_ratio",) + NAMES + ("levenshtein",))
    assert re.search(r'__all__ = \[[^\]]*' + order + r'[^\]]*"sorensen_dice",\s*"extract",\s*\]', src)
    for fn in NAMES:
        doc = re.search(r'def %s\(expr: IntoExpr, other: IntoExpr\) -> pl\.Expr:\n    """(.*?)"""' % fn, src, re.S).group(1)
        assert ("fuzz.WRatio" if fn == "wratio" else "fuzz." + fn) in doc and "/ 100" in doc and "upstream polars-strsim" in doc


def test_headers_declare_and_library_exports_the_weighted_symbols(L):
    hdr = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    api = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    for n, i in zip(NAMES, IDS):
        assert "POLARS_PLUGIN_DECLARE(%s)" % n in hdr
        assert re.search(r"STRSIM_%s\s*=\s*%d\b" % (n.upper(), i), api)
        assert hasattr(L, "_polars_plugin_" + n) and hasattr(L, "_polars_plugin_field_" + n)
    assert re.search(r"#define STRSIM_ABI_VERSION 0x00010007u", api)
    assert "strsim_ctx_last_wratio_rows" in api and hasattr(L, "strsim_ctx_last_wratio_rows")
