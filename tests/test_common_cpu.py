"""Hamming, prefix, postfix and LCSseq without a GPU: the reference (common_ref) on the known answers, its LCS against
tests/indel_ref.py and its bit-parallel form; the host build of the kernels' shared code (strsim_common.h: the byte-window count per
kind, the end alignment, the two UTF-8 boundary rules, the lockstep walk) against brute force, as a library and as a stand-alone
program under AddressSanitizer and UBSan; the exported symbols and every argument error of the six entry points, before any device;
and the Python surfaces."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import common_ref as R
import indel_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "common_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
ERR_SHAPE, ERR_ARG = 1, 2
UNBOUNDED = 0xFFFFFFFF
SIM = ["strsim_common_device", "strsim_common_host"]
DIST = ["strsim_common_distance_device", "strsim_common_distance_host"]
COUNT = ["strsim_common_count_device", "strsim_common_count_host"]
ENTRY_POINTS = SIM + DIST + COUNT
FUNCS = [k + s for k in R.KINDS for s in ("", "_distance", "_similarity")]


# ---- the reference ------------------------------------------------------------------------------------------------------------

def test_common_reference_known_answers():
    for kind, a, b, c in R.KNOWN:
        assert R.count(kind, a, b) == c == R.count(kind, b, a), (kind, a, b)
    for kind, a, b, d in R.KNOWN_DISTANCES:
        assert R.distance(kind, a, b) == d == R.distance(kind, b, a), (kind, a, b)
    assert R.score("lcs_seq", "AGGTAB", "GXTXAYB") == 1.0 - 3.0 / 7.0
    # bytewise answers would differ: one or two common bytes, no common character
    assert "é".encode()[:1] == "è".encode()[:1] and "€".encode()[:2] == "₭".encode()[:2]
    assert "é".encode()[1:] == "©".encode()[1:] and "€".encode()[1:] == "Ⴌ".encode()[1:]
    assert sum(x == y for x, y in zip("éa".encode(), "ea".encode())) == 0
    for kind in R.KINDS:
        assert R.count(kind, "", "") == 0 and R.score(kind, "", "") == 1.0
        assert R.count(kind, "", "abc") == 0 and R.distance(kind, "abc", "") == 3 and R.score(kind, "", "abc") == 0.0
        assert R.count(kind, "a\0b", "a\0b") == 3 and R.count(kind, "\0", "") == 0  # a NUL is a character
        assert R.score(kind, "abc", "abc") == 1.0
    assert R.clamp(3, 2) == 3 and R.clamp(2, 2) == 2 and R.clamp(5, None) == 5 and R.clamp(1, 0) == 1 and R.clamp(0, 0) == 0
    assert list(R.clamp(np.array([0, 3, 9], dtype=np.uint32), 3)) == [0, 3, 4]


def random_pairs(seed, n, alphabet, hi):
    rng = random.Random(seed)
    out = []
    for r in range(n):
        a = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, hi)))
        b = R.edited(rng, a, alphabet, rng.randint(0, 4)) if r % 3 else "".join(rng.choice(alphabet) for _ in range(rng.randint(0, hi)))
        out.append((a, b))
    return out


def test_common_reference_lcs_against_indel_ref():
    for alphabet, hi in (("ab", 14), ("abcd", 40), ("aé日😀\0", 30)):
        for a, b in random_pairs(5, 700, alphabet, hi):
            l = R.lcs_seq(a, b)
            assert 2 * l == len(a) + len(b) - indel_ref.distance(a, b), (a, b)
            assert l == indel_ref.lcs(a, b) == R.lcs_bits(a, b) == R.lcs_bits(b, a), (a, b)
    cref = indel_ref.CRef()
    rng = random.Random(2)
    a = "".join(rng.choice("abcdeé") for _ in range(900))
    b = R.edited(rng, a, "abcdeé", 60)[:870]
    assert R.count("lcs_seq", a, b) == R.lcs_bits(a, b) == cref.lcs(a, b)  # (count() takes the bit-parallel form beyond 64 characters)
    assert 2 * R.lcs_bits(a, b) == len(a) + len(b) - cref.distance(a, b)


def test_common_reference_relations():
    for a, b in random_pairs(9, 2000, "abcde", 24):
        c = {k: R.count(k, a, b) for k in R.KINDS}
        assert c["prefix"] <= c["hamming"] <= c["lcs_seq"] <= min(len(a), len(b)), (a, b)
        assert c["postfix"] <= c["lcs_seq"], (a, b)
        assert c["postfix"] == R.prefix(a[::-1], b[::-1])
        for k in R.KINDS:
            assert R.count(k, b, a) == c[k] and R.distance(k, a, b) >= abs(len(a) - len(b))


# ---- the host build of the kernels' shared code ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def build_dir():
    d = tempfile.TemporaryDirectory(prefix="common_harness_")
    yield d.name
    d.cleanup()


@pytest.fixture(scope="module")
def H(build_dir):
    so = os.path.join(build_dir, "libcommon_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    L.common_lane_max_c.restype = u32
    for name in ("common_lane_c", "common_wave_c"):
        getattr(L, name).restype = u32
        getattr(L, name).argtypes = [C.c_int, C.c_char_p, u32, C.c_char_p, u32]
    L.common_lane_row_c.restype = u32
    L.common_lane_row_c.argtypes = [C.c_int, u32, u32, C.c_int, u32]
    L.common_distance_c.restype = u64
    L.common_distance_c.argtypes = [u64, u64, u64]
    L.common_clamp_c.restype = u32
    L.common_clamp_c.argtypes = [u64, u32]
    L.common_score_c.restype = C.c_double
    L.common_score_c.argtypes = [u64, u64, u64]
    L.common_sweep_lane_random_c.argtypes = [u32, u32]
    L.common_sweep_lockstep_c.argtypes = [u32, u32, u32, u32]
    return L


def lane(H, kind, a, b):
    a, b = a.encode(), b.encode()
    return H.common_lane_c(R.KINDS.index(kind), a, len(a), b, len(b))


def wave(H, kind, a, b):
    a, b = a.encode(), b.encode()
    return H.common_wave_c(R.KINDS.index(kind), a, len(a), b, len(b))


def test_common_harness_known_answers(H):
    assert H.common_lane_max_c() == 32
    for kind, a, b, c in R.KNOWN:
        if kind == "lcs_seq":
            continue
        for x, y in ((a, b), (b, a)):
            assert wave(H, kind, x, y) == c, (kind, x, y)
            if x.isascii() and y.isascii():
                assert lane(H, kind, x, y) == c, (kind, x, y)
    for kind in ("hamming", "prefix", "postfix"):
        for a, b in (("\0", ""), ("\0", "\0\0"), ("a\0", "\0a"), ("\0" * 32, "\0" * 31), ("\0" * 31 + "a", "\0" * 32), ("x" * 32, "x" * 32)):
            assert lane(H, kind, a, b) == R.count(kind, a, b) == wave(H, kind, a, b), (kind, a, b)


def test_common_harness_every_length_pair_and_difference_position(H):
    # every length pair 0..33 over three letters, the first difference at every byte position: the lane core up to 32, the walks always
    assert H.common_sweep_lengths_c() == 0


def test_common_harness_random_lane_pairs(H):
    assert H.common_sweep_lane_random_c(3000, 11) == 0


def test_common_harness_utf8_boundary_rules(H):
    # all pairs of strings of up to 3 characters over a, é, è, ©, €, ₭, U+10AC and 😀, all three walks
    assert H.common_sweep_utf8_c() == 0
    for a, b in (("aé", "aè"), ("a€", "a₭"), ("éa", "©a"), ("€a", "Ⴌa"), ("😀", "😁"), ("é", "éé"), ("€€", "€")):
        for kind in ("hamming", "prefix", "postfix"):
            assert wave(H, kind, a, b) == R.count(kind, a, b), (kind, a, b)


def test_common_harness_lockstep_walk(H):
    assert H.common_sweep_lockstep_c(400, 60, 140, 5) == 0
    rng = random.Random(4)
    for _ in range(200):
        a = "".join(rng.choice("aé日😀") for _ in range(rng.randint(60, 140)))
        b = R.edited(rng, a, "aé日😀", rng.randint(0, 5))
        for kind in ("hamming", "prefix", "postfix"):
            assert wave(H, kind, a, b) == R.count(kind, a, b), (kind, a, b)
    # the cursors drift by more than a chunk: 200 one-byte characters against 200 two-byte ones with a common tail
    a, b = "a" * 200 + "xyz", "é" * 200 + "xyz"
    assert wave(H, "hamming", a, b) == 3 == wave(H, "postfix", a, b) and wave(H, "prefix", a, b) == 0


def test_common_harness_pieces_rows_and_results(H):
    assert H.common_sweep_pieces_c() == 0
    NONE, WAVE, CUT, RUN = 0, 1, 2, 3
    assert H.common_lane_row_c(0, 1, 1, 1, UNBOUNDED) == NONE
    assert H.common_lane_row_c(1, 32, 32, 1, UNBOUNDED) == RUN and H.common_lane_row_c(1, 33, 0, 1, UNBOUNDED) == WAVE
    assert H.common_lane_row_c(1, 0, 33, 1, 0) == WAVE and H.common_lane_row_c(1, 5, 5, 0, 3) == WAVE
    assert H.common_lane_row_c(1, 10, 5, 1, 4) == CUT and H.common_lane_row_c(1, 10, 5, 1, 5) == RUN and H.common_lane_row_c(1, 3, 3, 1, 0) == RUN
    assert H.common_distance_c(4, 6, 7) == 3 and H.common_distance_c(0, 0, 0) == 0 and H.common_distance_c(0, 0, 5) == 5
    assert H.common_clamp_c(3, 2) == 3 and H.common_clamp_c(2, 2) == 2 and H.common_clamp_c(7, UNBOUNDED) == 7 and H.common_clamp_c(1, 0) == 1
    for c, la, lb in ((4, 6, 7), (0, 0, 0), (0, 0, 3), (3, 3, 3), (1, 2, 3), (41, 42, 43)):
        assert H.common_score_c(c, la, lb) == R.normalise(max(la, lb) - c, la, lb)


def test_common_harness_under_sanitizers(build_dir):
    # the same harness as a stand-alone program with its own main, under AddressSanitizer and UBSan, run once
    exe = os.path.join(build_dir, "common_harness_san")
    # (the sanitizer runtimes are linked statically: the program needs nothing from its environment)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-DCOMMON_HARNESS_MAIN", "-I", CSRC, "-o", exe, HARNESS])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "common_harness: 0 mismatches" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name in SIM + COUNT:
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, vp, u64]
    for name in DIST:
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, u32, vp, u64]
    L.strsim_abi_version.restype = C.c_uint32
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_measure_supported.argtypes = [C.c_int, C.c_int]
    L.strsim_last_error_message.restype = C.c_char_p
    return L


def test_common_adds_no_measure_and_keeps_the_abi_version(L):
    assert L.strsim_abi_version() == 0x00010007
    for unassigned in (5, 7, 27, 28):
        assert L.strsim_measure_supported(unassigned, 0) == 0


def test_common_symbols_are_exported_and_declared(L):
    hdr = " ".join(open(os.path.join(ROOT, "include", "strsim_amd.h")).read().split())
    assert "enum { STRSIM_COMMON_HAMMING = 0, STRSIM_COMMON_PREFIX = 1, STRSIM_COMMON_POSTFIX = 2, STRSIM_COMMON_LCSSEQ = 3 };" in hdr
    cols = "const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows, const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows, "
    for name in SIM:
        assert "STRSIM_API int %s(strsim_ctx_t *ctx, int kind, %sdouble *out, uint64_t out_rows);" % (name, cols) in hdr
    for name in DIST:
        assert "STRSIM_API int %s(strsim_ctx_t *ctx, int kind, %suint32_t max_distance, uint32_t *out, uint64_t out_rows);" % (name, cols) in hdr
    for name in COUNT:
        assert "STRSIM_API int %s(strsim_ctx_t *ctx, int kind, %suint32_t *out, uint64_t out_rows);" % (name, cols) in hdr
    plugin = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    names = list(ENTRY_POINTS)
    assert len(FUNCS) == 12
    for fn in FUNCS:
        assert "POLARS_PLUGIN_DECLARE(%s)\n" % fn in plugin
        names += ["_polars_plugin_" + fn, "_polars_plugin_field_" + fn]
    for name in names:
        assert getattr(L, name) is not None


def call(L, name, kind=0, a_rows=1, b_rows=1, out_rows=1, null=None, k=UNBOUNDED):
    ao = (C.c_uint32 * 4)(0, 1, 2, 3)
    av = (C.c_uint8 * 4)(97, 98, 99, 100)
    out = (C.c_uint64 * 4)(*([0x5A5A5A5A5A5A5A5A] * 4))
    p = {"a_off": C.addressof(ao), "a_val": C.addressof(av), "b_off": C.addressof(ao), "b_val": C.addressof(av), "out": C.addressof(out)}
    if null:
        p[null] = None
    args = [None, kind, p["a_off"], p["a_val"], a_rows, p["b_off"], p["b_val"], b_rows]
    args += [k] if "distance" in name else []
    rc = getattr(L, name)(*args, p["out"], out_rows)
    assert list(out) == [0x5A5A5A5A5A5A5A5A] * 4  # nothing written
    return rc


@pytest.mark.parametrize("name", ENTRY_POINTS)
@pytest.mark.parametrize("case,kw,code,msg", [
    ("kind_low", dict(kind=-1), ERR_ARG, "{name}: unknown kind -1 (STRSIM_COMMON_HAMMING, _PREFIX, _POSTFIX or _LCSSEQ: 0..3)"),
    ("kind_high", dict(kind=4), ERR_ARG, "{name}: unknown kind 4 (STRSIM_COMMON_HAMMING, _PREFIX, _POSTFIX or _LCSSEQ: 0..3)"),
    ("kind_before_shape", dict(kind=9, a_rows=2, b_rows=3, out_rows=2), ERR_ARG, "{name}: unknown kind 9"),
    ("shape", dict(a_rows=2, b_rows=3, out_rows=2), ERR_SHAPE, "must have the same length"),
    ("out_rows", dict(kind=3, a_rows=3, b_rows=1, out_rows=2), ERR_ARG, "{name}: out_rows=2 but the inputs produce 3 rows"),
    ("null_a_offsets", dict(null="a_off"), ERR_ARG, "{name}: NULL buffer"),
    ("null_a_values", dict(kind=1, null="a_val"), ERR_ARG, "{name}: NULL buffer"),
    ("null_b_offsets", dict(kind=2, null="b_off"), ERR_ARG, "{name}: NULL buffer"),
    ("null_b_values", dict(kind=3, null="b_val"), ERR_ARG, "{name}: NULL buffer"),
    ("null_out", dict(null="out"), ERR_ARG, "{name}: NULL buffer"),
    ("null_ctx", dict(), ERR_ARG, "{name}: ctx is NULL"),
    ("null_ctx_every_kind", dict(kind=3), ERR_ARG, "{name}: ctx is NULL"),
    ("null_ctx_literal", dict(a_rows=1, b_rows=3, out_rows=3, k=0), ERR_ARG, "{name}: ctx is NULL"),
    ("null_ctx_zero_rows", dict(a_rows=0, b_rows=0, out_rows=0, null="out"), ERR_ARG, "{name}: ctx is NULL"),
])
def test_common_argument_errors_need_no_device(L, name, case, kw, code, msg):
    # the arguments are checked in the order kind, rows, buffers, and the context last
    assert call(L, name, **kw) == code
    got = L.strsim_last_error_message().decode()
    want = msg.format(name=name)
    assert got.startswith(want) if "{name}" in msg else want in got, got


# ---- Python surfaces --------------------------------------------------------------------------------------------------------------

def test_common_python_surface():
    import strsim_amd
    from strsim_amd.context import Context
    assert strsim_amd.COMMON_KINDS == R.KINDS and "COMMON_KINDS" in strsim_amd.__all__
    assert set(FUNCS) <= set(strsim_amd.__all__)
    for fn in FUNCS:
        assert callable(getattr(strsim_amd, fn))
    for m in ("common_host", "common_device", "common_distance_host", "common_distance_device", "common_count_host", "common_count_device"):
        assert callable(getattr(Context, m))
    for kind in R.KINDS:
        assert kind not in strsim_amd.MEASURES and kind not in strsim_amd.DISTANCE_MEASURES
    # ValueError before a context is made or touched (there is no device here to make one on)
    for fn in ("hamming_distance", "lcs_seq_distance", "prefix_distance", "postfix_distance"):
        for bad in (-1, 2 ** 32):
            with pytest.raises(ValueError, match="max_distance=.* is outside"):
                getattr(strsim_amd, fn)(["a"], ["b"], max_distance=bad)
    for fn in FUNCS:
        with pytest.raises(ValueError, match="same length"):
            getattr(strsim_amd, fn)(["a", "b"], ["a", "b", "c"])
    ctx = Context.__new__(Context)  # (no handle: the arguments are refused before it is used)
    off, val = strsim_amd.pack_strings(["a"])
    for m in ("common_host", "common_distance_host", "common_count_host"):
        with pytest.raises(ValueError, match="unknown kind 'levenshtein'"):
            getattr(ctx, m)("levenshtein", off, val, off, val)
    with pytest.raises(ValueError, match="unknown kind 3"):
        ctx.common_device(3, None, None, None, None)
    with pytest.raises(ValueError, match="max_distance=-1 is outside"):
        ctx.common_distance_host("hamming", off, val, off, val, max_distance=-1)
    with pytest.raises(ValueError, match="max_distance=-2 is outside"):
        ctx.common_distance_device("prefix", None, None, None, None, max_distance=-2)
    # the character counts that pad=False compares
    off, val = strsim_amd.pack_strings(["", "abc", "éa", "日本語", "😀", "a\0b"])
    assert list(strsim_amd._char_lengths(off, val)) == [0, 3, 2, 3, 1, 3]


def test_common_polars_wrappers_source():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    for kind in R.KINDS:
        assert "def %s(expr: IntoExpr, other: IntoExpr) -> pl.Expr:" % kind in src
        assert "def %s_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:" % kind in src
        assert "def %s_similarity(expr: IntoExpr, other: IntoExpr) -> pl.Expr:" % kind in src
        assert '_similarity("%s", expr, other)' % kind in src
        assert '_distance("%s_distance", expr, other, max_distance)' % kind in src
        assert '_distance("%s_similarity", expr, other, None)' % kind in src
        for fn in (kind, kind + "_distance", kind + "_similarity"):
            assert '"%s",' % fn in src
    assert "pl.when(a.str.len_chars() == b.str.len_chars())" in src  # (no pad argument: the signatures above)


def test_common_plugin_fields():
    pa = pytest.importorskip("pyarrow")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    from strsim_amd import arrow_host
    for kind in R.KINDS:
        assert arrow_host.field_plugin(kind, ("left", "right")) == ("left", pa.float64())
        assert arrow_host.field_plugin(kind + "_distance", ("l", "r", "max_distance")) == ("l", pa.uint32())
        assert arrow_host.field_plugin(kind + "_similarity", ("l", "r")) == ("l", pa.uint32())
