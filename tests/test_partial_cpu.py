"""Partial ratio (measure 10) without a GPU: the brute-force model against the known answers and its C form, the host build of the
lane tier's sweep core and of the wave tier's per-window cores (strsim_partial.h) against the model, strsim_measure_supported, the
refusals of the other entry points, the argument errors of strsim_partial_alignment_*, and the Python and polars_strsim surfaces."""
import ctypes as C
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import indel_ref
import partial_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "partial_lane_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
PARTIAL = 10
PAIRWISE, BEST_MATCH, CODEC = 0, 1, 2


@pytest.fixture(scope="module")
def cref():
    return R.CRef()


@pytest.fixture(scope="module")
def lane():
    d = tempfile.TemporaryDirectory(prefix="partial_lane_")
    so = os.path.join(d.name, "libpartial_lane.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    u32 = C.c_uint32
    L.partial_lane_host.restype = C.c_int
    L.partial_lane_host.argtypes = [C.c_char_p, u32, C.c_char_p, u32, u32, u32, u32, C.c_int, C.c_void_p, C.c_void_p]
    L.partial_wave_host.restype = C.c_int
    L.partial_wave_host.argtypes = [C.c_void_p, u32, C.c_void_p, u32, C.c_void_p]
    L.partial_score_host.restype = C.c_double
    L.partial_score_host.argtypes = [u32, u32, u32]
    L.partial_wave_words_host.restype = C.c_uint64
    L.partial_wave_words_host.argtypes = [C.c_uint64, C.c_uint64]
    yield L
    d.cleanup()


def _lane(lane, a: bytes, b: bytes, mmax=None, nmax=None, m2max=None, second_any=0):
    m, n = min(len(a), len(b)), max(len(a), len(b))
    score = C.c_double(-1.0)
    span = (C.c_uint32 * 4)(9, 9, 9, 9)
    ok = lane.partial_lane_host(a, len(a), b, len(b), m if mmax is None else mmax, n if nmax is None else nmax,
                                m if m2max is None else m2max, second_any, C.byref(score), span)
    assert ok == 1
    return (score.value,) + tuple(span)


# ---- the model ----

@pytest.mark.parametrize("a,b,score,sa,sb", R.KNOWN)
def test_partial_known_answers(cref, a, b, score, sa, sb):
    assert R.partial(a, b) == (score,) + sa + sb
    assert cref.partial(a, b) == (score,) + sa + sb
    # exchanged: the same score, the spans exchanged -- except that for equal lengths the tie rule names a the needle
    got = R.partial(b, a)
    assert got[0] == score and cref.partial(b, a) == got
    if len(a) != len(b):
        assert got[1:] == sb + sa


def test_partial_windows_order_and_count():
    for m in range(1, 9):
        for n in range(m, 14):
            w = R.windows(m, n)
            assert len(w) == n + m - 1 and len(set(w)) == len(w)
            assert w == sorted(w, key=lambda se: (se[1], se[0]))
            assert all(0 <= s < e <= n and e - s <= m for s, e in w)
            assert sum(1 for s, e in w if e - s == m) == n - m + 1


def test_partial_score_is_symmetric_and_python_equals_c(cref):
    rng = random.Random(11)
    A, B = [], []
    for alphabet in ("ab", "abcdefgh", "abcdefghijklmnopqrstuvwxyz", "aé€😀b"):
        for _ in range(150):
            A.append("".join(rng.choice(alphabet) for _ in range(rng.randint(0, 12))))
            B.append("".join(rng.choice(alphabet) for _ in range(rng.randint(0, 12))))
    s, sp, ties, flag = cref.batch(A, B)
    s2, _, _, _ = cref.batch(B, A)
    assert (s.view(np.uint64) == s2.view(np.uint64)).all()
    for r, (a, b) in enumerate(zip(A, B)):
        want = R.partial(a, b)
        assert (float(s[r]),) + tuple(int(x) for x in sp[r]) == want, (a, b)
        assert int(ties[r]) == R.count_at_max(a, b), (a, b)
        assert bool(flag[r]) == R.second_direction_wins(a, b)
        assert R.partial(b, a)[0] == want[0]
        if a and b and len(a) <= len(b):
            assert cref.P(a, b) == R._P(a, b)


def test_partial_can_be_lower_than_indel():
    """n > m: the whole haystack is not a window."""
    assert R.partial("ab", "axb")[0] < indel_ref.score("ab", "axb")


# ---- the lane tier's core ----

@pytest.mark.parametrize("alphabet", ["ab", "abcdefgh"])
def test_lane_core_every_length_pair(lane, cref, alphabet):
    rng = random.Random(len(alphabet))
    A, B = [], []
    for la in range(0, 33):
        for lb in range(0, 33):
            for _ in range(2):
                A.append("".join(rng.choice(alphabet) for _ in range(la)))
                B.append("".join(rng.choice(alphabet) for _ in range(lb)))
    s, sp, _, flag = cref.batch(A, B)
    assert flag.sum() > 10  # (rows where b as the needle wins are in the frame)
    for r, (a, b) in enumerate(zip(A, B)):
        want = (float(s[r]),) + tuple(int(x) for x in sp[r])
        assert _lane(lane, a.encode(), b.encode()) == want, (a, b)
        # the bounds of a wave whose other lanes are longer, and whose second pass runs for another lane's sake
        assert _lane(lane, a.encode(), b.encode(), 32, 32, 32, 1) == want, (a, b)
        m, n = min(len(a), len(b)), max(len(a), len(b))
        assert _lane(lane, a.encode(), b.encode(), min(32, m + 3), min(32, n + 5), min(32, m + 1), r & 1) == want, (a, b)


def test_lane_core_nul_bytes(lane, cref):
    """A NUL byte is a character; zero padding never matches it."""
    rng = random.Random(5)
    cases = [(b"\0", b"\0\0\0"), (b"a\0", b"\0a\0\0"), (b"\0\0", b"ab"), (b"\0" * 32, b"\0" * 31), (b"a", b"\0" * 32), (b"\0", b"a" * 32)]
    for _ in range(400):
        cases.append((bytes(rng.choice(b"\0a") for _ in range(rng.randint(0, 32))), bytes(rng.choice(b"\0a") for _ in range(rng.randint(0, 32)))))
    A = [a.decode("latin-1") for a, _ in cases]
    B = [b.decode("latin-1") for _, b in cases]
    s, sp, _, _ = cref.batch(A, B)
    for r, (a, b) in enumerate(cases):
        want = (float(s[r]),) + tuple(int(x) for x in sp[r])
        assert _lane(lane, a, b) == want, (a, b)
        assert _lane(lane, a, b, 32, 32, 32, 1) == want, (a, b)


# ---- the wave tier's per-window cores ----

@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130])
def test_wave_cores(lane, cref, m):
    rng = random.Random(m)
    for alphabet, n in (("ab", m), ("ab", m + 1), ("abcd", m + 70), ("ab", 2 * m + 3), ("aé€😀", m + 9)):
        s = "".join(rng.choice(alphabet) for _ in range(m))
        t = "".join(rng.choice(alphabet) for _ in range(n))
        if rng.random() < 0.5 and n > m + 4:  # plant the needle with one edit
            k = rng.randrange(0, n - m)
            t = t[:k] + s[:m // 2] + "x" + s[m // 2 + 1:] + t[k + m:]
        x = np.array([ord(c) for c in s], dtype=np.uint32)
        y = np.array([ord(c) for c in t], dtype=np.uint32)
        out = np.zeros(3, dtype=np.uint32)
        assert lane.partial_wave_host(x.ctypes.data, m, y.ctypes.data, len(t), out.ctypes.data) == 1
        l, wl, start = (int(v) for v in out)
        assert (lane.partial_score_host(l, wl, m), start, start + wl) == cref.P(s, t), (m, n, alphabet)


def test_wave_table_words(lane):
    assert lane.partial_wave_words_host(64, 100) == 200
    assert lane.partial_wave_words_host(65, 100) == 100 + 128 + 4
    assert lane.partial_wave_words_host(65, 101) == 101 + 128 + 1 + 4


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
    for name in ("strsim_partial_alignment_device", "strsim_partial_alignment_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, u64]
    for name in ("strsim_pairs_device", "strsim_pairs_device_small", "strsim_pairs_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, vp, u64]
    for name in ("strsim_distance_device", "strsim_distance_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, vp, u64]
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
    return L


def test_partial_measure_supported(L):
    assert L.strsim_measure_supported(PARTIAL, PAIRWISE) == 1
    assert L.strsim_measure_supported(PARTIAL, BEST_MATCH) == 0
    assert L.strsim_measure_supported(PARTIAL, CODEC) == 0
    assert L.strsim_measure_supported(PARTIAL, 3) == 0
    for m in (5, 7, 9, 11, 12, 100, -1):
        for e in (PAIRWISE, BEST_MATCH, CODEC):
            assert L.strsim_measure_supported(m, e) == 0, (m, e)
    assert L.strsim_abi_version() == 0x00010007


def test_other_entry_points_refuse_the_partial_ratio_before_any_device(L):
    for name in ("strsim_pairs_device", "strsim_pairs_device_small", "strsim_pairs_host"):
        assert getattr(L, name)(None, PARTIAL, None, None, 1, None, None, 1, None, 1) == 2
        assert b"ctx is NULL" in L.strsim_last_error_message()  # (the measure itself is accepted)
    for name in ("strsim_pairs_device", "strsim_pairs_device_small"):
        for m in (9, 11):
            ctx_stand_in = C.create_string_buffer(8)  # (never dereferenced: the measure is refused first)
            assert getattr(L, name)(ctx_stand_in, m, None, None, 1, None, None, 1, None, 1) == 2
            assert b"unknown measure" in L.strsim_last_error_message()
    for name in ("strsim_best_match_device", "strsim_best_match_host"):
        assert getattr(L, name)(None, PARTIAL, None, None, 0, None, None, 0, 1, 0.0, None, None) == 2
        assert b"measure" in L.strsim_last_error_message()
    for name in ("strsim_nearest_device", "strsim_nearest_host"):
        assert getattr(L, name)(None, PARTIAL, None, None, 0, None, None, 0, 1, 1, None, None) == 2
        assert b"measure" in L.strsim_last_error_message()
    for name in ("strsim_distance_device", "strsim_distance_host"):
        assert getattr(L, name)(None, PARTIAL, None, None, 0, None, None, 0, 1, None, 0) == 2
        msg = L.strsim_last_error_message()
        assert b"measure 10 has no distance" in msg and b"STRSIM_INDEL" in msg
    out = C.c_void_p()
    ctx_stand_in = C.create_string_buffer(8)  # (never dereferenced: the measure is refused first)
    assert L.strsim_codec_create(ctx_stand_in, PARTIAL, 32, C.byref(out)) == 2
    assert b"bad measure" in L.strsim_last_error_message() and not out.value


@pytest.mark.parametrize("entry", ["strsim_partial_alignment_device", "strsim_partial_alignment_host"])
def test_alignment_argument_errors_without_a_device(L, entry):
    f = getattr(L, entry)
    off = np.array([0, 1, 2], dtype=np.uint32)
    val = np.frombuffer(b"ab", dtype=np.uint8).copy()
    score = np.zeros(2, dtype=np.float64)
    span = np.zeros(8, dtype=np.uint32)
    o, v, s, p = off.ctypes.data, val.ctypes.data, score.ctypes.data, span.ctypes.data
    assert f(None, o, v, 2, o, v, 3, s, p, 2) == 1  # shape
    assert L.strsim_last_error_message() == b"Inputs must have the same length, or one of them must be a Utf8 literal."
    assert f(None, o, v, 2, o, v, 2, s, p, 3) == 2  # out_rows
    assert b"out_rows" in L.strsim_last_error_message()
    for args in ((None, v, o, v, s, p), (o, None, o, v, s, p), (o, v, None, v, s, p), (o, v, o, None, s, p), (o, v, o, v, None, p),
                 (o, v, o, v, s, None)):
        assert f(None, args[0], args[1], 2, args[2], args[3], 2, args[4], args[5], 2) == 2
        assert b"NULL buffer" in L.strsim_last_error_message()
    assert f(None, o, v, 2, o, v, 2, s, p, 2) == 2  # every argument right: the NULL context
    assert b"ctx is NULL" in L.strsim_last_error_message()
    assert f(None, o, v, 1, o, v, 2, s, p, 2) == 2  # a literal on the left: shape ok, then the context
    assert b"ctx is NULL" in L.strsim_last_error_message()
    assert f(None, None, None, 0, None, None, 0, None, None, 0) == 2  # zero rows: nothing to check but the context


# ---- the Python surfaces ----

def test_partial_python_surface_without_a_device(L):
    import strsim_amd as S
    assert S.MEASURE_ID["partial_ratio"] == PARTIAL and S.PARTIAL_MEASURES == ("partial_ratio",)
    assert S.MEASURES == ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")
    assert S.EXTRA_MEASURES == ("osa",) and S.DISTANCE_MEASURES == ("levenshtein", "osa") and S.INDEL_MEASURES == ("indel",)
    assert S.measure_supported("partial_ratio") and not S.measure_supported("partial_ratio", "best_match")
    assert not S.measure_supported("partial_ratio", "codec")
    for name in ("partial_ratio", "partial_ratio_alignment", "PARTIAL_MEASURES"):
        assert name in S.__all__ and hasattr(S, name)
    assert hasattr(S.Context, "partial_alignment_host") and hasattr(S.Context, "partial_alignment_device")
    with pytest.raises(ValueError, match="no distance"):
        S.distance("partial_ratio", ["a"], ["b"])
    with pytest.raises(ValueError, match="no distance"):
        S.nearest("partial_ratio", ["a"], ["b"])
    with pytest.raises(ValueError, match="no best match"):
        S.best_match("partial_ratio", ["a"], ["b"])


def test_polars_wrapper_source_lists_the_partial_ratio():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert re.search(r'__all__ = \[[^\]]*"indel_distance"[^\]]*"indel"[^\]]*"partial_ratio"[^\]]*"partial_ratio_alignment"', src)
    for fn in ("partial_ratio", "partial_ratio_alignment"):
        doc = re.search(r'def %s\(expr: IntoExpr, other: IntoExpr\) -> pl\.Expr:\n    """(.*?)"""' % fn, src, re.S).group(1)
        assert "fuzz.partial_ratio" in doc and "/ 100" in doc and "upstream polars-strsim" in doc
    doc = re.search(r'def partial_ratio\(.*?"""(.*?)"""', src, re.S).group(1)
    assert "prefixes" in doc and "suffixes" in doc and "substring of m characters" in doc


def test_partial_field_functions():
    pa = pytest.importorskip("pyarrow")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    from strsim_amd import arrow_host
    assert arrow_host.field_plugin("partial_ratio", ("left", "right")) == ("left", pa.float64())
    name, dtype = arrow_host.field_plugin("partial_ratio_alignment", ("left", "right"))
    assert name == "left"
    assert dtype == pa.struct([("score", pa.float64()), ("src_start", pa.uint32()), ("src_end", pa.uint32()),
                               ("dest_start", pa.uint32()), ("dest_end", pa.uint32())])


def test_headers_declare_and_library_exports_the_partial_symbols(L):
    hdr = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    assert "POLARS_PLUGIN_DECLARE(partial_ratio)" in hdr and "POLARS_PLUGIN_DECLARE(partial_ratio_alignment)" in hdr
    api = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    assert re.search(r"STRSIM_PARTIAL_RATIO\s*=\s*10\b", api)
    assert "strsim_partial_alignment_device" in api and "strsim_partial_alignment_host" in api
    for sym in ("_polars_plugin_partial_ratio", "_polars_plugin_partial_ratio_alignment", "_polars_plugin_field_partial_ratio",
                "_polars_plugin_field_partial_ratio_alignment", "strsim_partial_alignment_device", "strsim_partial_alignment_host"):
        assert hasattr(L, sym), sym
