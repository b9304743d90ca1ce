"""q-gram similarity without a GPU: the model (qgram_ref) on the known answers, against the oracle at q = 1 and under its relations;
the exported symbols and every argument error of the two entry points, before any device; the Python surfaces; the plugin's field
functions; and the host build of the kernels' shared code (strsim_qgram.h: the lane core and the table rules) against brute force."""
import ctypes as C
import math
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import gen
import oracle_lib as O
import qgram_ref as R
from golden_data import reference_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "qgram_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
ERR_SHAPE, ERR_ARG = 1, 2

KNOWN, KNOWN_ANY = R.KNOWN, R.KNOWN_ANY

def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# ---- the model ----------------------------------------------------------------------------------------------------------------

def test_qgram_model_known_answers():
    for a, b, q, multiset, cnt, scores in KNOWN:
        if cnt is not None:
            assert R.counts(a, b, q, multiset) == cnt
        for kind, want in scores.items():
            assert R.score(kind, a, b, q, multiset) == want, (a, b, q, multiset, kind)
    for a, b, q, want in KNOWN_ANY:
        for kind in R.KINDS:
            for multiset in (True, False):
                assert R.score(kind, a, b, q, multiset) == want


@pytest.mark.parametrize("kind", ["jaccard", "sorensen_dice"])
def test_qgram_model_at_q1_is_the_oracle_bit_for_bit(kind):
    rows = [r for r in reference_vectors() if r[0] == kind]
    assert len(rows) > 20
    A, B = [r[2] for r in rows], [r[3] for r in rows]
    A1, B1 = gen.pairs(31, 3000, gen.ASCII_LOWER, 0, 40)
    A2, B2 = gen.pairs(32, 1500, gen.MIXED, 0, 90)
    A, B = A + A1 + A2, B + B1 + B2
    want = O.batch_strings(kind, A, B, 4)
    got = R.batch(kind, A, B, 1, True)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, [(A[i], B[i], got[i], want[i]) for i in bad[:5]]


def test_qgram_model_relations():
    rng = random.Random(5)
    for _ in range(3000):
        alphabet = rng.choice(["ab", "abc", gen.ASCII_LOWER, gen.MIXED])
        a, b = gen.rand_string(rng, alphabet, 0, 12), gen.rand_string(rng, alphabet, 0, 12)
        for q in (1, 2, 3):
            for multiset in (True, False):
                s = {k: R.score(k, a, b, q, multiset) for k in R.KINDS}
                for k in R.KINDS:
                    assert s[k] == R.score(k, b, a, q, multiset)  # symmetry
                    assert 0.0 <= s[k] <= 1.0
                i, na, nb = R.counts(a, b, q, multiset)
                if na and nb:
                    assert s["jaccard"] <= s["sorensen_dice"] <= s["cosine"] <= s["overlap"], (a, b, q, multiset, s)
            ga, gb = R.grams(a, q), R.grams(b, q)
            if len(set(ga)) == len(ga) and len(set(gb)) == len(gb):  # no gram repeats: the set score is the multiset score
                for k in R.KINDS:
                    assert R.score(k, a, b, q, True) == R.score(k, a, b, q, False)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name in ("strsim_qgram_device", "strsim_qgram_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, u32, u32, vp, vp, u64, vp, vp, u64, vp, u64]
    L.strsim_abi_version.restype = C.c_uint32
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_measure_supported.argtypes = [C.c_int, C.c_int]
    L.strsim_last_error_message.restype = C.c_char_p
    return L


def test_qgram_adds_no_measure_and_keeps_the_abi_version(L):
    assert L.strsim_abi_version() == 0x00010007
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    assert "enum { STRSIM_QGRAM_JACCARD = 0, STRSIM_QGRAM_SORENSEN_DICE = 1, STRSIM_QGRAM_OVERLAP = 2, STRSIM_QGRAM_COSINE = 3 };" in hdr
    assert re.search(r"#define STRSIM_QGRAM_SET 1u", hdr)
    for unassigned in (5, 7, 27, 28):
        assert L.strsim_measure_supported(unassigned, 0) == 0


def test_qgram_symbols_are_exported(L):
    names = ["strsim_qgram_device", "strsim_qgram_host"]
    hdr = open(os.path.join(ROOT, "include", "polars_plugin_abi.h")).read()
    for kind in R.KINDS:
        names += ["_polars_plugin_qgram_" + kind, "_polars_plugin_field_qgram_" + kind]
        assert "POLARS_PLUGIN_DECLARE(qgram_%s)" % kind in hdr
    for name in names:
        assert getattr(L, name) is not None


def _qgram_call(L, name, kind=1, q=2, flags=0, a_rows=1, b_rows=1, out_rows=1, null=None):
    ao = (C.c_uint32 * 4)(0, 1, 2, 3)
    av = (C.c_uint8 * 4)(97, 98, 99, 100)
    out = (C.c_double * 4)()
    p = {"a_off": C.addressof(ao), "a_val": C.addressof(av), "b_off": C.addressof(ao), "b_val": C.addressof(av), "out": C.addressof(out)}
    if null:
        p[null] = None
    return getattr(L, name)(None, kind, q, flags, p["a_off"], p["a_val"], a_rows, p["b_off"], p["b_val"], b_rows, p["out"], out_rows)


@pytest.mark.parametrize("name", ["strsim_qgram_device", "strsim_qgram_host"])
@pytest.mark.parametrize("case,kw,code,msg", [
    ("kind4", dict(kind=4), ERR_ARG, "{name}: unknown kind 4 (STRSIM_QGRAM_JACCARD, _SORENSEN_DICE, _OVERLAP or _COSINE: 0..3)"),
    ("kind_minus1", dict(kind=-1), ERR_ARG, "{name}: unknown kind -1 (STRSIM_QGRAM_JACCARD, _SORENSEN_DICE, _OVERLAP or _COSINE: 0..3)"),
    ("q0", dict(q=0), ERR_ARG, "{name}: q=0 is outside 1..3"),
    ("q4", dict(q=4), ERR_ARG, "{name}: q=4 is outside 1..3"),
    ("flags2", dict(flags=2), ERR_ARG, "{name}: unknown flag bits 0x2 (STRSIM_QGRAM_SET is the only flag)"),
    ("flags_high", dict(flags=0x80000001), ERR_ARG, "{name}: unknown flag bits 0x80000000 (STRSIM_QGRAM_SET is the only flag)"),
    ("kind_before_q", dict(kind=9, q=0, flags=6), ERR_ARG, "{name}: unknown kind 9"),
    ("q_before_flags", dict(q=7, flags=6), ERR_ARG, "{name}: q=7 is outside 1..3"),
    ("flags_before_shape", dict(flags=4, a_rows=2, b_rows=3, out_rows=2), ERR_ARG, "{name}: unknown flag bits 0x4"),
    ("shape", dict(a_rows=2, b_rows=3, out_rows=2), ERR_SHAPE, "must have the same length"),
    ("out_rows", dict(a_rows=3, b_rows=1, out_rows=2), ERR_ARG, "{name}: out_rows=2 but the inputs produce 3 rows"),
    ("null_a_offsets", dict(null="a_off"), ERR_ARG, "{name}: NULL buffer"),
    ("null_a_values", dict(null="a_val"), ERR_ARG, "{name}: NULL buffer"),
    ("null_b_offsets", dict(null="b_off"), ERR_ARG, "{name}: NULL buffer"),
    ("null_b_values", dict(null="b_val"), ERR_ARG, "{name}: NULL buffer"),
    ("null_out", dict(null="out"), ERR_ARG, "{name}: NULL buffer"),
    ("null_ctx", dict(), ERR_ARG, "{name}: ctx is NULL"),
    ("null_ctx_set_mode_q3", dict(kind=3, q=3, flags=1, a_rows=1, b_rows=3, out_rows=3), ERR_ARG, "{name}: ctx is NULL"),
])
def test_qgram_argument_errors_need_no_device(L, name, case, kw, code, msg):
    # the arguments are checked in the order kind, q, flags, rows, buffers, and the context last
    assert _qgram_call(L, name, **kw) == code
    got = L.strsim_last_error_message().decode()
    want = msg.format(name=name)
    assert got.startswith(want) if "{name}" in msg else want in got, got


@pytest.mark.parametrize("name", ["strsim_qgram_device", "strsim_qgram_host"])
def test_qgram_zero_rows_is_a_no_op_without_a_context(L, name):
    assert _qgram_call(L, name, a_rows=0, b_rows=0, out_rows=0, null="out") == ERR_ARG  # (ctx is NULL: the checks come first)
    assert "ctx is NULL" in L.strsim_last_error_message().decode()


# ---- Python surfaces and plugin fields ------------------------------------------------------------------------------------------

def test_qgram_python_surface():
    import strsim_amd
    from strsim_amd.context import Context
    assert strsim_amd.QGRAM_KINDS == R.KINDS == ("jaccard", "sorensen_dice", "overlap", "cosine")
    assert {"qgram", "QGRAM_KINDS"} <= set(strsim_amd.__all__) and callable(strsim_amd.qgram)
    assert callable(Context.qgram_host) and callable(Context.qgram_device)
    # ValueError before a context is made or touched (there is no device here to make one on)
    for bad in ("levenshtein", "dice", 0, None):
        with pytest.raises(ValueError, match="unknown q-gram kind"):
            strsim_amd.qgram(bad, ["a"], ["b"])
    for bad in (0, 4, -1, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="is outside 1 .. 3"):
            strsim_amd.qgram("jaccard", ["a"], ["b"], q=bad)
    ctx = Context.__new__(Context)  # (no handle: the arguments are refused before it is used)
    off, val = strsim_amd.pack_strings(["a"])
    with pytest.raises(ValueError, match="unknown q-gram kind"):
        ctx.qgram_host("jaro", off, val, off, val)
    with pytest.raises(ValueError, match="q=4 is outside"):
        ctx.qgram_host("cosine", off, val, off, val, q=4)
    with pytest.raises(ValueError, match="q=0 is outside"):
        ctx.qgram_device("cosine", None, None, None, None, q=0)


def test_qgram_polars_wrappers_source():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "__init__.py")).read()
    for kind in R.KINDS:
        assert "def qgram_%s(expr: IntoExpr, other: IntoExpr, q: int = 2, multiset: bool = True) -> pl.Expr:" % kind in src
        assert '"qgram_%s"' % kind in src
    assert "pl.lit(q, dtype=pl.UInt32)" in src and 'function_name="qgram_" + kind' in src


def test_qgram_polars_wrappers_refuse_bad_arguments():
    pytest.importorskip("polars")
    import polars_strsim as ps
    for fn in (ps.qgram_jaccard, ps.qgram_sorensen_dice, ps.qgram_overlap, ps.qgram_cosine):
        for bad in (0, 4, "2", 2.0, None):
            with pytest.raises(ValueError, match="is outside 1 .. 3"):
                fn("a", "b", q=bad)
    with pytest.raises(ValueError, match="unknown q-gram kind"):
        ps._qgram("jaro", "a", "b", 2, True)


@pytest.mark.parametrize("kind", R.KINDS)
def test_qgram_field_is_float64_named_after_first_input(kind):
    pa = pytest.importorskip("pyarrow")
    from strsim_amd import arrow_host
    assert arrow_host.field_plugin("qgram_" + kind, ("left", "right", "q")) == ("left", pa.float64())
    assert arrow_host.field_plugin("qgram_" + kind, ("l", "r", "q", "set")) == ("l", pa.float64())


# ---- host build of the kernels' shared code -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def H():
    d = tempfile.TemporaryDirectory(prefix="qgram_harness_")
    so = os.path.join(d.name, "libqgram_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    L = C.CDLL(so)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.qgram_lane.restype = C.c_int
    L.qgram_lane.argtypes = [C.c_char_p, u32, C.c_char_p, u32, u32, C.c_int, C.c_int, u32, vp]
    L.qgram_lane_sweep.restype = u64
    L.qgram_lane_sweep.argtypes = [C.c_char_p, u32, u64, u32, C.c_int, vp]
    L.qgram_table.restype = C.c_int
    L.qgram_table.argtypes = [vp, u32, vp, u32, u32, C.c_int, C.c_int, vp]
    L.qgram_table_sweep.restype = u64
    L.qgram_table_sweep.argtypes = [u64]
    L.qgram_score_c.restype = C.c_double
    L.qgram_score_c.argtypes = [C.c_int, u64, u64, u64, C.c_int]
    L.qgram_key_c.restype = u64
    L.qgram_key_c.argtypes = [u32, u32, u32]
    L.qgram_table_slots_c.restype = u64
    L.qgram_table_slots_c.argtypes = [u64]
    L.qgram_wave_slot_words_c.restype = u64
    L.qgram_wave_slot_words_c.argtypes = [u64, u64]
    yield L
    d.cleanup()


ALPHABETS = {"one": b"a", "two": b"ab", "eight": b"abcdefgh", "ascii_with_nul": bytes(range(128)), "nul_and_a": b"\0a"}


@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
@pytest.mark.parametrize("multiset", [True, False])
@pytest.mark.parametrize("q", [1, 2, 3])
def test_qgram_lane_core_every_length_pair(H, alphabet, q, multiset):
    # 0..64 x 0..64, each mask width that holds the pair, the wave's longest text at and above the pair's
    first = (C.c_uint32 * 9)()
    al = ALPHABETS[alphabet]
    bad = H.qgram_lane_sweep(al, len(al), 100 + q, q, 0 if multiset else 1, C.addressof(first))
    assert bad == 0, "la=%d lb=%d words=%d got %s want %s" % (first[0], first[1], first[2], list(first[3:6]), list(first[6:9]))


def _lane(H, a, b, q, multiset, words, slack=0):
    out = (C.c_uint32 * 3)()
    rc = H.qgram_lane(a, len(a), b, len(b), q, 0 if multiset else 1, words, slack, C.addressof(out))
    return None if rc else tuple(out)


def test_qgram_lane_core_against_the_model(H):
    # ties the harness's brute force to qgram_ref: known answers, a real NUL against padding, random rows at both widths
    for a, b, q, multiset, cnt, _ in KNOWN:
        if cnt is not None:
            assert _lane(H, a.encode(), b.encode(), q, multiset, 1) == cnt == _lane(H, a.encode(), b.encode(), q, multiset, 2, 7)
    for q in (1, 2, 3):
        for multiset in (True, False):
            a, b = b"a\0", b"a\0\0"
            want = R.counts(a.decode(), b.decode(), q, multiset)
            assert _lane(H, a, b, q, multiset, 1, 3) == want == _lane(H, a, b, q, multiset, 2)
            assert _lane(H, b, a, q, multiset, 1) == (want[0], want[2], want[1])
    rng = random.Random(9)
    for _ in range(1500):
        al = rng.choice(["a", "ab", "abc", "abcdefgh", "ab\0"])
        a, b = gen.rand_string(rng, al, 0, 64), gen.rand_string(rng, al, 0, 64)
        q, multiset = rng.choice([1, 2, 3]), rng.random() < 0.5
        want = R.counts(a, b, q, multiset)
        assert _lane(H, a.encode(), b.encode(), q, multiset, 2, rng.choice([0, 9])) == want, (a, b, q, multiset)
        if len(a) <= 32 and len(b) <= 32:
            assert _lane(H, a.encode(), b.encode(), q, multiset, 1) == want, (a, b, q, multiset)
    assert _lane(H, b"a" * 33, b"a", 1, True, 1) is None  # (does not fit one mask word)


def _table(H, va, vb, q, multiset, count_bytes):
    a = np.asarray(list(va) + [0], dtype=np.uint32)
    b = np.asarray(list(vb) + [0], dtype=np.uint32)
    out = (C.c_uint64 * 5)()
    rc = H.qgram_table(a.ctypes.data, len(va), b.ctypes.data, len(vb), q, 0 if multiset else 1, count_bytes, C.addressof(out))
    assert rc == 0
    return tuple(out)


def test_qgram_table_rules(H):
    assert H.qgram_table_sweep(3) == 0  # random values, both count widths, colliding keys, the key nearest the empty value
    # against the model, over strings that hold 2-, 3- and 4-byte characters
    rng = random.Random(21)
    for _ in range(400):
        a, b = gen.rand_string(rng, "ab" + gen.MIXED, 0, 70), gen.rand_string(rng, "abé\U0001d11e", 0, 70)
        q, multiset = rng.choice([1, 2, 3]), rng.random() < 0.5
        got = _table(H, [ord(c) for c in a], [ord(c) for c in b], q, multiset, rng.choice([4, 8]))
        assert got[:3] == R.counts(a, b, q, multiset), (a, b, q, multiset)
    # load at most 1/2 in a power of two of at least 64 slots
    for grams in (0, 1, 32, 33, 64, 65, 1024, 1025, 2048, 2049, 5000):
        slots = H.qgram_table_slots_c(grams)
        assert slots >= max(64, 2 * grams) and slots & (slots - 1) == 0 and (slots == 64 or slots < 4 * grams)
    # no key is the empty value: three times the largest 21-bit value keeps bit 63 clear
    assert H.qgram_key_c(0x1FFFFF, 0x1FFFFF, 0x1FFFFF) == (1 << 63) - 1
    assert H.qgram_key_c(0x10FFFF, 1, 2) == 0x10FFFF | (1 << 21) | (2 << 42)
    # a scratch slot holds the keys, the counts (64 bits each) and the values of one string, in an even number of words
    assert H.qgram_wave_slot_words_c(2049, 3000) == 4 * 8192 + 3004


def test_qgram_score_rules(H):
    for kind, name in enumerate(R.KINDS):
        assert H.qgram_score_c(kind, 0, 0, 0, 1) == 1.0  # rule 1
        assert H.qgram_score_c(kind, 0, 0, 5, 0) == 0.0 and H.qgram_score_c(kind, 0, 5, 0, 0) == 0.0  # rule 2
        assert H.qgram_score_c(kind, 7, 7, 7, 0) == 1.0  # equal strings with grams: every formula gives 1.0 itself
    for i, na, nb in [(1, 4, 4), (2, 3, 3), (2, 2, 2), (3, 7, 11), (5, 5, 64), (1, 63, 64), (17, 1000, 1999)]:
        assert H.qgram_score_c(0, i, na, nb, 0) == i / (na + nb - i)
        assert H.qgram_score_c(1, i, na, nb, 0) == (2.0 * i) / (na + nb)
        assert H.qgram_score_c(2, i, na, nb, 0) == i / min(na, nb)
        assert H.qgram_score_c(3, i, na, nb, 0) == i / math.sqrt(float(na * nb))
    # the product of the cosine is formed in 64-bit integers
    assert H.qgram_score_c(3, 1 << 20, 1 << 31, 1 << 31, 0) == float(1 << 20) / math.sqrt(float(1 << 62))
