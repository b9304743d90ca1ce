"""Unrestricted Damerau-Levenshtein without a GPU: the reference (damerau_ref) against the definition -- a search over single edits --
against its C form, on the known answers and under its relations; the host build of the kernels' shared code (strsim_damerau.h: the
lane core as k_dl_lane runs it, the strip walk as k_dl_wave runs it) against the reference; the exported symbols and every argument
error of the four entry points, before any device; the Python surfaces; and the shares of the GPU suite's lane frame."""
import ctypes as C
import itertools
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import damerau_ref as R
import distance_ref
import osa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "damerau_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
ERR_SHAPE, ERR_ARG = 1, 2
UNBOUNDED = 0xFFFFFFFF
ENTRY_POINTS = ["strsim_damerau_device", "strsim_damerau_host", "strsim_damerau_distance_device", "strsim_damerau_distance_host"]


@pytest.fixture(scope="module")
def cref():
    return R.CRef()


# ---- the reference ------------------------------------------------------------------------------------------------------------

def edits(s, alphabet, cap):
    """every string one edit away from s, none longer than cap"""
    out = set()
    for i in range(len(s)):
        out.add(s[:i] + s[i + 1:])
        for c in alphabet:
            out.add(s[:i] + c + s[i + 1:])
    if len(s) < cap:
        for i in range(len(s) + 1):
            for c in alphabet:
                out.add(s[:i] + c + s[i:])
    for i in range(len(s) - 1):
        out.add(s[:i] + s[i + 1] + s[i] + s[i + 2:])
    out.discard(s)
    return out


def test_dl_reference_is_the_shortest_edit_sequence():
    # breadth first over single edits from every string over abc of length 0..4, strings capped at 4: 121 x 121 = 14 641 pairs
    alphabet, cap = "abc", 4
    words = ["".join(p) for n in range(cap + 1) for p in itertools.product(alphabet, repeat=n)]
    assert len(words) == 121
    near = {w: edits(w, alphabet, cap) for w in words}
    pairs = 0
    for src in words:
        dist = {src: 0}
        frontier = [src]
        while frontier:
            nxt = []
            for w in frontier:
                for v in near[w]:
                    if v not in dist:
                        dist[v] = dist[w] + 1
                        nxt.append(v)
            frontier = nxt
        assert len(dist) == len(words)
        for dst in words:
            assert R.distance(src, dst) == dist[dst], (src, dst)
            pairs += 1
    assert pairs == 14641


def test_dl_reference_known_answers(cref):
    for a, b, d, d_osa in R.KNOWN:
        assert R.distance(a, b) == d == R.distance(b, a), (a, b)
        assert cref.distance(a, b) == d == cref.distance(b, a), (a, b)
        assert osa_ref.distance(a, b) == d_osa, (a, b)
    for a, b, s in R.KNOWN_SCORES:
        assert R.score(a, b) == s == cref.score(a, b), (a, b)
    assert R.score("", "") == 1.0 and R.score("abc", "abc") == 1.0 and R.score("", "abc") == 0.0
    # the restricted distance is no metric, this one is
    assert osa_ref.distance("ca", "ac") + osa_ref.distance("ac", "abc") < osa_ref.distance("ca", "abc")
    assert R.distance("ca", "ac") + R.distance("ac", "abc") >= R.distance("ca", "abc")


def random_pairs(seed, n, alphabet, hi):
    rng = random.Random(seed)
    out = []
    for r in range(n):
        a = "".join(rng.choice(alphabet) for _ in range(rng.randrange(hi + 1)))
        if r % 3 == 0:
            b = "".join(rng.choice(alphabet) for _ in range(rng.randrange(hi + 1)))
        elif r % 3 == 1:
            b = R.gapped(rng, a, rng.randrange(1, 4), alphabet)
        else:
            b = R.swapped(rng, R.gapped(rng, a, 1, alphabet), 2)
        out.append((a, b))
    return out


def test_dl_c_reference_equals_the_python_one(cref):
    for alphabet, hi in (("ab", 12), ("abcd", 40), ("aé日😀\0", 30)):
        for a, b in random_pairs(5, 1500, alphabet, hi):
            assert cref.distance(a, b) == R.distance(a, b), (a, b)
    # (only the touched entries of the table are reset: a second, unrelated pair after a long one)
    assert cref.distance("😀" * 300 + "xy", "😀" * 300 + "yzx") == 2 and cref.distance("ca", "abc") == 2


def test_dl_relations_on_a_random_frame(cref):
    less = 0
    for a, b in random_pairs(9, 3000, "abcde", 24):
        d = cref.distance(a, b)
        lev, osa = distance_ref.distance("levenshtein", a, b, None), osa_ref.distance(a, b)
        assert lev >= osa >= d >= abs(len(a) - len(b)), (a, b, lev, osa, d)
        assert d == cref.distance(b, a), (a, b)
        less += d < osa
    assert less > 100


# ---- the host build of the kernels' shared code ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="damerau_harness_")
    so = os.path.join(d.name, "libdamerau_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    for name in ("dl_lane_max_c", "dl_wave_lds_cols_c", "dl_wave_small_cols_c"):
        getattr(L, name).restype = u32
    L.dl_wave_slot_words_c.restype = u64
    L.dl_wave_slot_words_c.argtypes = [u64]
    L.dl_lane_c.restype = u32
    L.dl_lane_c.argtypes = [C.c_char_p, u32, C.c_char_p, u32, C.c_int, u32, u32, u32]
    L.dl_walk_c.restype = u32
    L.dl_walk_c.argtypes = [vp, u32, vp, u32, u32, u32]
    L.dl_lane_row_c.restype = u32
    L.dl_lane_row_c.argtypes = [C.c_int, u32, u32, C.c_int, u32]
    L.dl_result_u32_c.restype = u32
    L.dl_result_u32_c.argtypes = [u64, u64, u64, u32]
    L.dl_result_f64_c.restype = C.c_double
    L.dl_result_f64_c.argtypes = [u64, u64, u64]
    yield L
    d.cleanup()


def lane(H, a, b, lit=0, pslack=0, tslack=0, stride=1):
    a, b = a.encode(), b.encode()
    return H.dl_lane_c(a, len(a), b, len(b), lit, pslack, tslack, stride)


def walk(H, a, b, cap=None, slot_cols=0):
    x = np.array([ord(c) for c in a] or [0], dtype=np.uint32)
    y = np.array([ord(c) for c in b] or [0], dtype=np.uint32)
    return H.dl_walk_c(x.ctypes.data, len(a), y.ctypes.data, len(b), H.dl_wave_lds_cols_c() if cap is None else cap, slot_cols)


def test_dl_constants(H):
    assert H.dl_lane_max_c() == 32 and H.dl_wave_small_cols_c() == 256 and H.dl_wave_lds_cols_c() == 2048
    assert H.dl_wave_slot_words_c(2049) == 5 * 2049


def test_dl_lane_core_every_length_pair(H, cref):
    rng = random.Random(3)
    M = H.dl_lane_max_c()
    for la in range(M + 1):
        for lb in range(M + 1):
            a = "".join(rng.choice("abc") for _ in range(la))
            b = R.gapped(rng, a, rng.randrange(3), "abc")
            b = (b + "".join(rng.choice("abc") for _ in range(M)))[:lb] if rng.randrange(2) else R.swapped(rng, b, 1)[:lb].ljust(lb, "c")
            want = cref.distance(a, b)
            for lit in (0, 1, 2):
                # (loop bounds beyond the lane's own strings, as in a wave with longer rows; its records at a stride)
                assert lane(H, a, b, lit, rng.randrange(4), rng.randrange(4), 1 + rng.randrange(4)) == want, (a, b, lit)


def test_dl_lane_core_known_and_nul(H, cref):
    M = H.dl_lane_max_c()
    for a, b, d, _ in R.KNOWN:
        if a.isascii() and b.isascii() and max(len(a), len(b)) <= M:
            assert lane(H, a, b) == d == lane(H, b, a), (a, b)
    for a, b in (("\0", ""), ("\0", "\0\0"), ("a\0", "\0a"), ("a\0b", "\0xa"), ("\0" * 32, "\0" * 31), ("ab" * 16, "ba" * 16),
                 ("x" * 30 + "ca", "x" * 29 + "abc")):
        assert lane(H, a, b) == cref.distance(a, b), (a, b)
    for a, b in random_pairs(11, 3000, "abcdefghijklmnopqrstuvwxyz", M):
        b = b[:M]
        assert lane(H, a, b) == cref.distance(a, b), (a, b)


def test_dl_lane_row_classes_and_results(H):
    NONE, WAVE, CUT, RUN = 0, 1, 2, 3
    assert H.dl_lane_row_c(0, 1, 1, 1, UNBOUNDED) == NONE
    assert H.dl_lane_row_c(1, 32, 32, 1, UNBOUNDED) == RUN and H.dl_lane_row_c(1, 33, 0, 1, UNBOUNDED) == WAVE
    assert H.dl_lane_row_c(1, 0, 33, 1, 0) == WAVE and H.dl_lane_row_c(1, 5, 5, 0, 3) == WAVE
    assert H.dl_lane_row_c(1, 10, 5, 1, 4) == CUT and H.dl_lane_row_c(1, 10, 5, 1, 5) == RUN and H.dl_lane_row_c(1, 3, 3, 1, 0) == RUN
    assert H.dl_result_u32_c(3, 9, 9, 2) == 3 and H.dl_result_u32_c(2, 9, 9, 2) == 2 and H.dl_result_u32_c(0, 9, 9, 0) == 0
    assert H.dl_result_u32_c(7, 9, 9, UNBOUNDED) == 7 and H.dl_result_u32_c(1, 9, 9, 0) == 1
    for d, la, lb in ((2, 2, 3), (2, 42, 43), (2, 65, 66), (0, 0, 0), (3, 0, 3)):
        assert H.dl_result_f64_c(d, la, lb) == R.normalise(d, la, lb)


@pytest.mark.parametrize("rows", [63, 64, 65, 127, 128, 129])
def test_dl_strip_walk_at_the_strip_edges(H, cref, rows):
    rng = random.Random(rows)
    for cols in (1, 5, 62, 63, 64, 65, 66, 126, 127, 128, 129):
        if cols > rows:
            continue
        a = "".join(rng.choice("abcé") for _ in range(rows))
        b = R.gapped(rng, a[:cols], 3, "abcé")[:cols]
        want = cref.distance(a, b)
        assert walk(H, a, b) == want == walk(H, b, a), (rows, cols)
        # the boundary row in the scratch layout, from a small "LDS" limit on
        assert walk(H, a, b, cap=16, slot_cols=max(cols, 17)) == want, (rows, cols)


def test_dl_strip_walk_edit_across_the_strip_boundary(H, cref):
    # x y -> y z x with x at row 64 and y at row 65 (1-based) of the longer string; and the three characters across columns 64 | 65
    base = "".join("abcdefgh"[i % 8] for i in range(140))
    for i in (62, 63, 64, 126, 127, 128):
        b = R.gapped_at(base, i, "q")
        for a, c in ((base, b), (b, base), (base[:130], b), (b[:131], base)):
            want = cref.distance(a, c)
            assert walk(H, a, c) == want, (i, len(a), len(c))
        assert cref.distance(base, b) == 2 and osa_ref.distance(base, b) == 3


def test_dl_strip_walk_edit_across_the_lds_scratch_boundary(H, cref):
    # the shorter string has 2 047 / 2 048 (boundary row in LDS) or 2 049+ values (in scratch), the edit sits on columns 2 047 .. 2 049
    cap = H.dl_wave_lds_cols_c()
    rng = random.Random(1)
    base = "".join(rng.choice("abcdefgh") for _ in range(cap + 70))
    for i in (cap - 2, cap - 1, cap):
        b = R.gapped_at(base, i, "q")
        for n in (cap - 1, cap, cap + 1, cap + 5):
            a, c = base[:n + 66], b[:n]
            assert walk(H, a, c, slot_cols=max(n, cap + 1)) == cref.distance(a, c), (i, n)


def test_dl_strip_walk_random(H, cref):
    for a, b in random_pairs(13, 300, "ab日", 200):
        assert walk(H, a, b) == cref.distance(a, b), (a, b)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name in ENTRY_POINTS[:2]:
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, u64]
    for name in ENTRY_POINTS[2:]:
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64, u32, vp, u64]
    L.strsim_abi_version.restype = C.c_uint32
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_measure_supported.argtypes = [C.c_int, C.c_int]
    L.strsim_last_error_message.restype = C.c_char_p
    return L


def test_dl_adds_no_measure_and_keeps_the_abi_version(L):
    assert L.strsim_abi_version() == 0x00010007
    for unassigned in (5, 7, 27, 28):
        assert L.strsim_measure_supported(unassigned, 0) == 0


def test_dl_symbols_are_exported_and_declared(L):
    hdr = " ".join(open(os.path.join(ROOT, "include", "strsim_amd.h")).read().split())
    cols = "const uint32_t *a_offsets, const uint8_t *a_values, uint64_t a_rows, const uint32_t *b_offsets, const uint8_t *b_values, uint64_t b_rows, "
    for name in ENTRY_POINTS[:2]:
        assert "STRSIM_API int %s(strsim_ctx_t *ctx, %sdouble *out, uint64_t out_rows);" % (name, cols) in hdr
    for name in ENTRY_POINTS[2:]:
        assert "STRSIM_API int %s(strsim_ctx_t *ctx, %suint32_t max_distance, uint32_t *out, uint64_t out_rows);" % (name, cols) in hdr
    plugin = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    names = list(ENTRY_POINTS)
    for fn in ("damerau_levenshtein", "damerau_levenshtein_distance"):
        assert "POLARS_PLUGIN_DECLARE(%s)\n" % fn in plugin
        names += ["_polars_plugin_" + fn, "_polars_plugin_field_" + fn]
    for name in names:
        assert getattr(L, name) is not None


def call(L, name, a_rows=1, b_rows=1, out_rows=1, null=None, k=UNBOUNDED):
    ao = (C.c_uint32 * 4)(0, 1, 2, 3)
    av = (C.c_uint8 * 4)(97, 98, 99, 100)
    out = (C.c_uint64 * 4)(*([0x5A5A5A5A5A5A5A5A] * 4))
    p = {"a_off": C.addressof(ao), "a_val": C.addressof(av), "b_off": C.addressof(ao), "b_val": C.addressof(av), "out": C.addressof(out)}
    if null:
        p[null] = None
    args = [None, p["a_off"], p["a_val"], a_rows, p["b_off"], p["b_val"], b_rows]
    args += [k] if "distance" in name else []
    rc = getattr(L, name)(*args, p["out"], out_rows)
    assert list(out) == [0x5A5A5A5A5A5A5A5A] * 4  # nothing written
    return rc


@pytest.mark.parametrize("name", ENTRY_POINTS)
@pytest.mark.parametrize("case,kw,code,msg", [
    ("shape", dict(a_rows=2, b_rows=3, out_rows=2), ERR_SHAPE, "must have the same length"),
    ("out_rows", dict(a_rows=3, b_rows=1, out_rows=2), ERR_ARG, "{name}: out_rows=2 but the inputs produce 3 rows"),
    ("null_a_offsets", dict(null="a_off"), ERR_ARG, "{name}: NULL buffer"),
    ("null_a_values", dict(null="a_val"), ERR_ARG, "{name}: NULL buffer"),
    ("null_b_offsets", dict(null="b_off"), ERR_ARG, "{name}: NULL buffer"),
    ("null_b_values", dict(null="b_val"), ERR_ARG, "{name}: NULL buffer"),
    ("null_out", dict(null="out"), ERR_ARG, "{name}: NULL buffer"),
    ("null_ctx", dict(), ERR_ARG, "{name}: ctx is NULL"),
    ("null_ctx_literal", dict(a_rows=1, b_rows=3, out_rows=3, k=0), ERR_ARG, "{name}: ctx is NULL"),
    ("null_ctx_zero_rows", dict(a_rows=0, b_rows=0, out_rows=0, null="out"), ERR_ARG, "{name}: ctx is NULL"),
])
def test_dl_argument_errors_need_no_device(L, name, case, kw, code, msg):
    # the arguments are checked in the order rows, buffers, and the context last
    assert call(L, name, **kw) == code
    got = L.strsim_last_error_message().decode()
    want = msg.format(name=name)
    assert got.startswith(want) if "{name}" in msg else want in got, got


# ---- Python surfaces --------------------------------------------------------------------------------------------------------------

def test_dl_python_surface():
    import strsim_amd
    from strsim_amd.context import Context
    assert {"damerau_levenshtein", "damerau_levenshtein_distance"} <= set(strsim_amd.__all__)
    for m in ("damerau_host", "damerau_device", "damerau_distance_host", "damerau_distance_device"):
        assert callable(getattr(Context, m))
    assert "damerau_levenshtein" not in strsim_amd.MEASURES and "damerau_levenshtein" not in strsim_amd.DISTANCE_MEASURES
    # ValueError before a context is made or touched (there is no device here to make one on)
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="max_distance=.* is outside"):
            strsim_amd.damerau_levenshtein_distance(["a"], ["b"], max_distance=bad)
    for fn in (strsim_amd.damerau_levenshtein, strsim_amd.damerau_levenshtein_distance):
        with pytest.raises(ValueError, match="same length"):
            fn(["a", "b"], ["a", "b", "c"])
    ctx = Context.__new__(Context)  # (no handle: the arguments are refused before it is used)
    off, val = strsim_amd.pack_strings(["a"])
    with pytest.raises(ValueError, match="max_distance=-1 is outside"):
        ctx.damerau_distance_host(off, val, off, val, max_distance=-1)
    with pytest.raises(ValueError, match="max_distance=-2 is outside"):
        ctx.damerau_distance_device(None, None, None, None, max_distance=-2)


def test_dl_polars_wrappers_source():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    assert "def damerau_levenshtein(expr: IntoExpr, other: IntoExpr) -> pl.Expr:" in src
    assert "def damerau_levenshtein_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:" in src
    assert '_similarity("damerau_levenshtein", expr, other)' in src
    assert '_distance("damerau_levenshtein_distance", expr, other, max_distance)' in src
    assert '"damerau_levenshtein",' in src and '"damerau_levenshtein_distance",' in src


def test_dl_plugin_fields():
    pa = pytest.importorskip("pyarrow")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    from strsim_amd import arrow_host
    assert arrow_host.field_plugin("damerau_levenshtein", ("left", "right")) == ("left", pa.float64())
    assert arrow_host.field_plugin("damerau_levenshtein_distance", ("l", "r", "max_distance")) == ("l", pa.uint32())


# ---- the GPU suite's lane frame ---------------------------------------------------------------------------------------------------

def test_dl_lane_frame_shares(cref):
    A, B = R.lane_frame(random.Random(41), 4000, 32)
    assert all(len(a) <= 32 and len(b) <= 32 and a.isascii() and b.isascii() for a, b in zip(A, B))
    d = np.array([cref.distance(a, b) for a, b in zip(A, B)])
    d_osa = np.array([osa_ref.distance(a, b) for a, b in zip(A, B)])
    assert (d <= d_osa).all()
    assert (d < d_osa).mean() >= 0.25, (d < d_osa).mean()
    assert (d == 0).mean() <= 0.40, (d == 0).mean()
