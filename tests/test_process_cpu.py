"""default_process and processed scoring without a GPU: the model (tests/process_ref.py) against known answers, against the
whole-string Python form and against the facts the design rests on; the committed table against the model and against its
generator; the g++ build of the row functions of strsim_process.h against the model; the C ABI and the Python surfaces as far as
they go without a device."""
import ctypes as C
import os
import random
import subprocess
import sys
import tempfile
import unicodedata

import numpy as np
import pytest

import process_frames as F
import process_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "process_harness.cpp")
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
TABLE = os.path.join(CSRC, "strsim_process_table.h")
GENERATOR = os.path.join(ROOT, "tools", "gen_process_table.py")
NOT_LANE, GUARD_HIT = 0xFFFFFFFF, 0xFFFFFFFE
SCALARS = [c for c in range(0x110000) if not 0xD800 <= c <= 0xDFFF]


# ---- the model ----

def test_known_answers():
    assert R.default_process("Apple, Inc.") == "apple  inc"
    assert R.default_process("apple inc") == "apple inc"
    assert R.default_process("Ⱥ_Kİ\U00010400\U0001F600ẞ9\x00") == "ⱥ_ki\U00010428 ß9"
    assert R.default_process("!!!") == ""
    assert R.default_process("ÀÉ　x") == "àé x"
    assert R.default_process("") == "" and R.default_process(None) is None
    assert R.default_process("  a  b  ") == "a  b"
    # the two scores of the issue's pair, by hand: "apple  inc" (10) against "apple inc" (9): LCS 9, d = 1, 1 - 1/19
    import indel_ref
    import token_ref
    assert indel_ref.score("Apple, Inc.", "apple inc") == 0.7
    assert indel_ref.score(R.default_process("Apple, Inc."), R.default_process("apple inc")) == 1 - 1 / 19 == 0.9473684210526316
    assert token_ref.token_sort_ratio("Apple, Inc.", "apple inc") == 0.7
    assert token_ref.token_sort_ratio(R.default_process("Apple, Inc."), R.default_process("apple inc")) == 1.0


def test_model_equals_the_whole_string_form_away_from_the_two_divergences():
    rng = random.Random(7)
    pool = [chr(c) for c in list(range(0x250)) + list(range(0x370, 0x530)) + [0x1E9E, 0x2126, 0x212A, 0x212B, 0x2000, 0x2028, 0x3000, 0x3042,
                                                                              0x6F22, 0xFF21, 0xFF41, 0x10400, 0x10428, 0x1D11E, 0x0301, 0x1F88]
            if c not in (0x03A3, 0x0130)]
    for _ in range(100000):
        s = "".join(rng.choice(pool) for _ in range(rng.randint(0, 12)))
        assert R.default_process(s) == R.default_process_whole(s), [hex(ord(c)) for c in s]


def test_the_two_documented_divergences():
    assert R.default_process("ΑΣ") == "ασ" and R.default_process_whole("ΑΣ") == "ας"
    assert R.default_process("İ") == "i" and R.default_process_whole("İ") == "i̇"


def test_facts_the_design_rests_on():
    growers, shrinkers = [], []
    for c in SCALARS:
        m = R.map_cp(c)
        assert R.map_cp(m) == m, hex(c)                                       # idempotent
        assert not chr(m).isspace() or m == 0x20, hex(c)                      # every surviving whitespace is U+0020
        if chr(c).isspace():
            assert m == 0x20, hex(c)
        a, b = len(chr(c).encode("utf-8")), len(chr(m).encode("utf-8"))
        if b > a:
            growers.append(c)
        if b < a and m != 0x20:   # (kept and shorter; whatever becomes a space shrinks to a byte)
            shrinkers.append(c)
    assert growers == [0x023A, 0x023E]
    assert len(chr(R.map_cp(0x023A)).encode("utf-8")) == 3 and len(chr(0x023A).encode("utf-8")) == 2
    assert {0x212A, 0x0130, 0x1E9E} <= set(shrinkers)
    if unicodedata.unidata_version == "13.0.0":
        assert len(shrinkers) == 23
    for c in range(0x80):                                                    # ASCII needs no table
        ch = chr(c)
        want = c + 32 if "A" <= ch <= "Z" else (c if ("a" <= ch <= "z" or "0" <= ch <= "9" or ch == "_") else 0x20)
        assert R.map_cp(c) == want
    assert R.map_cp(0xD800) == 0x20 and R.map_cp(0x110000) == 0x20


# ---- the table ----

@pytest.fixture(scope="module")
def L():
    L = C.CDLL(LIB)
    vp, u64 = C.c_void_p, C.c_uint64
    L.strsim_last_error_message.restype = C.c_char_p
    L.strsim_default_process_char.restype = C.c_uint32
    L.strsim_default_process_char.argtypes = [C.c_uint32]
    L.strsim_default_process_unicode_version.restype = C.c_char_p
    for name in ("strsim_default_process_device", "strsim_default_process_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64]
    for name in ("strsim_pairs_processed_device", "strsim_pairs_processed_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, C.c_int, vp, vp, u64, vp, vp, u64, vp, u64]
    L.strsim_ctx_last_process_wave_rows.restype = u64
    L.strsim_ctx_last_process_wave_rows.argtypes = [vp]
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_abi_version.restype = C.c_uint32
    return L


def _table_version():
    for line in open(TABLE):
        if line.startswith("#define STRSIM_PROCESS_UNICODE_VERSION"):
            return line.split('"')[1]
    raise AssertionError("no version in the table header")


def test_table_version_is_exported(L):
    assert L.strsim_default_process_unicode_version().decode() == _table_version()
    # out of range and surrogates: a space, whatever the Unicode version
    for cp in (0xD800, 0xDBFF, 0xDFFF, 0x110000, 0x1FFFFF, 0xFFFFFFFF):
        assert L.strsim_default_process_char(cp) == 0x20
    for cp, want in ((0x41, 0x61), (0x5F, 0x5F), (0, 0x20), (0x7F, 0x20), (0x023A, 0x2C65), (0x212A, 0x6B), (0x0130, 0x69), (0x03A3, 0x03C3),
                     (0x10400, 0x10428), (0x3000, 0x20), (0x6F22, 0x6F22), (0xA78D, 0x0265)):
        assert L.strsim_default_process_char(cp) == want, hex(cp)


@pytest.mark.skipif(unicodedata.unidata_version != _table_version(), reason="the table was generated from another Unicode version")
def test_table_equals_the_model_at_every_scalar_value(L):
    f = L.strsim_default_process_char
    bad = [hex(c) for c in range(0x110000) if f(c) != R.map_cp(c)]
    assert not bad, bad[:10]


@pytest.mark.skipif(unicodedata.unidata_version != _table_version(), reason="the table was generated from another Unicode version")
def test_generator_reproduces_the_committed_header():
    out = subprocess.run([sys.executable, GENERATOR, "-o", "-"], check=True, capture_output=True).stdout
    assert out == open(TABLE, "rb").read()


# ---- the g++ build of the row functions ----

@pytest.fixture(scope="module")
def rows():
    d = tempfile.mkdtemp(prefix="process_harness_")
    so = os.path.join(d, "process_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, HARNESS])
    H = C.CDLL(so)
    H.process_row_c.restype = C.c_uint32
    H.process_row_c.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p]
    H.process_map_c.restype = C.c_uint32
    H.process_map_c.argtypes = [C.c_uint32]
    H.process_map_ascii_word_c.restype = C.c_uint32
    H.process_map_ascii_word_c.argtypes = [C.c_uint32]
    H.process_lane_max_bytes_c.restype = C.c_uint32
    return H


def _row(H, b, tier, sa=0, da=0):
    out = C.create_string_buffer(len(b) + len(b) // 2 + 8)
    n = H.process_row_c(b, len(b), tier, sa, da, out)
    assert n != GUARD_HIT, (b, tier, sa, da)
    return None if n == NOT_LANE else out.raw[:n]


def test_lane_limit_is_the_frames_limit(rows):
    assert rows.process_lane_max_bytes_c() == F.LANE_MAX_BYTES


def test_ascii_word_map_equals_the_byte_map(rows):
    rng = random.Random(3)
    for b in range(0x80):   # every ASCII byte in every position, beside three others
        for k in range(4):
            other = [rng.randrange(0x80) for _ in range(4)]
            other[k] = b
            w = sum(x << (8 * i) for i, x in enumerate(other))
            want = sum(R.map_cp(x) << (8 * i) for i, x in enumerate(other))
            assert rows.process_map_ascii_word_c(w) == want, other


def test_row_functions_every_alignment_and_length(rows):
    """Lengths 0 .. 80 at every source and destination alignment, guard bytes around the destination (process_row_c reports a
    hit): the lane tier on ASCII, the wave tier on ASCII and on everything, both against the model."""
    rng = random.Random(5)
    everything = "".join(F.POOL)
    for n in range(81):
        ascii_row = "".join(rng.choice(F.ASCII_KEPT + F.ASCII_JUNK) for _ in range(n))
        mixed = F._to_bytes(rng, n, everything)
        junk_ends = (" ," * n)[:n // 3] + "".join(rng.choice(F.ASCII_KEPT) for _ in range(n - 2 * (n // 3))) + ("\0." * n)[:n // 3]
        for s in (ascii_row, mixed, junk_ends):
            b = s.encode("utf-8")
            assert len(b) == n
            want = R.default_process(s).encode("utf-8")
            for sa in range(4):
                for da in range(4):
                    assert _row(rows, b, 0, sa, da) == want, (s, sa, da)
                    got = _row(rows, b, 1, sa, da)
                    if F.is_lane_row(s):
                        assert got == want, (s, sa, da)
                    else:
                        assert got is None, (s, sa, da)


def test_row_functions_on_the_frame(rows):
    for s, want in zip(F.frame(), F.expected()):
        b = s.encode("utf-8")
        sa, da = len(b) % 4, (len(b) // 4) % 4
        assert _row(rows, b, 0, sa, da) == want.encode("utf-8"), s
        if F.is_lane_row(s):
            assert _row(rows, b, 1, sa, da) == want.encode("utf-8"), s


def test_truncated_sequences_stay_inside_the_row(rows):
    """A sequence cut off at the row's end: unspecified output, but equal to the textbook loop (missing continuation bytes count as
    zero), nothing read behind the row (the harness puts the row at the end of its block) and nothing written outside the output."""
    whole = ["Ⱥ", "K", "\U00010400", "\U0001D11E", "é", "　"]
    for c in whole:
        enc = c.encode("utf-8")
        for cut in range(1, len(enc)):
            for prefix in (b"", b"a", b"ab ", b"x" * 63, b"y" * 64, b" " * 65):
                b = prefix + enc[:cut]
                for sa in range(4):
                    for da in range(4):
                        assert _row(rows, b, 0, sa, da) == _row(rows, b, 2, sa, da), (b, sa, da)
    # nothing but lead bytes, or leads with too few continuation bytes: every lane of the wave on a start byte.  A lead byte
    # without its continuation bytes is a space on its own, so the output stays within bytes + bytes / 2 (and the wave's LDS words)
    for unit in (b"\xf0", b"\xe4", b"\xc8", b"\xf8", b"\xc8\xf0\xe4", b"\xf0\x90\xe4\x80\xc8", b"\xf0\x90\x90"):
        for n in (1, 63, 64, 65, 128, 200):
            b = (unit * n)[:n]
            for tail in (b"", b"a", b"\xc8\xba"):
                got = _row(rows, b + tail, 0, n % 4, (n // 4) % 4)
                assert got == _row(rows, b + tail, 2) and len(got) <= len(b + tail) * 3 // 2, (unit, n, tail)
    assert _row(rows, b"\xf0" * 64, 0) == b"" and _row(rows, b"x" + b"\xf0" * 64 + b"\xc8\xba", 0) == b"x" + b" " * 64 + "ⱥ".encode()
    for b in (b"\x80", b"\xbf\xbf\xbf", b"a\x80b", b"\xff", b"\xf8\x80\x80\x80\x80", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"):
        assert _row(rows, b, 0) == _row(rows, b, 2), b


# ---- the C ABI without a device ----

def test_symbols_and_abi_version(L):
    for name in ("strsim_default_process_char", "strsim_default_process_unicode_version", "strsim_default_process_device",
                 "strsim_default_process_host", "strsim_pairs_processed_device", "strsim_pairs_processed_host",
                 "strsim_ctx_last_process_wave_rows"):
        assert hasattr(L, name), name
    assert L.strsim_abi_version() == 0x00010007
    for e in (0, 1, 2):
        assert L.strsim_measure_supported(27, e) == 0 and L.strsim_measure_supported(28, e) == 0   # no measure id is added
    assert L.strsim_ctx_last_process_wave_rows(None) == 0
    header = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    assert "#define STRSIM_PROCESS_DEFAULT 1" in header
    assert "#define STRSIM_DEFAULT_PROCESS_CAPACITY(bytes) ((uint64_t)(bytes) + (uint64_t)(bytes) / 2u)" in header


@pytest.mark.parametrize("entry", ["strsim_default_process_device", "strsim_default_process_host"])
def test_default_process_argument_errors_without_a_device(L, entry):
    f = getattr(L, entry)
    off = np.array([0, 1, 2], dtype=np.uint32)
    val = np.frombuffer(b"ab", dtype=np.uint8).copy()
    out_off = np.zeros(3, dtype=np.uint32)
    out_val = np.zeros(3, dtype=np.uint8)
    o, v, oo, ov = off.ctypes.data, val.ctypes.data, out_off.ctypes.data, out_val.ctypes.data
    assert f(None, o, v, 1 << 32, oo, ov, 3) == 2
    assert b"rows in one call" in L.strsim_last_error_message()
    for args in ((None, v, oo, ov), (o, None, oo, ov), (o, v, None, ov), (o, v, oo, None)):
        assert f(None, args[0], args[1], 2, args[2], args[3], 3) == 2
        assert b"NULL buffer" in L.strsim_last_error_message()
    assert f(None, o, v, 2, oo, ov, 3) == 2          # every argument right: the NULL context, last
    assert b"ctx is NULL" in L.strsim_last_error_message()
    assert f(None, o, None, 0, oo, None, 0) == 2     # zero rows: the offsets and the context are all there is to check
    assert b"ctx is NULL" in L.strsim_last_error_message()


@pytest.mark.parametrize("entry", ["strsim_pairs_processed_device", "strsim_pairs_processed_host"])
def test_pairs_processed_argument_errors_without_a_device(L, entry):
    f = getattr(L, entry)
    off = np.array([0, 1, 2], dtype=np.uint32)
    val = np.frombuffer(b"ab", dtype=np.uint8).copy()
    out = np.zeros(2, dtype=np.float64)
    o, v, r = off.ctypes.data, val.ctypes.data, out.ctypes.data
    ctx_stand_in = C.create_string_buffer(8)  # (never dereferenced: every call below fails before the context is used)
    for processor in (0, 2, -1):
        assert f(ctx_stand_in, 8, processor, o, v, 2, o, v, 2, r, 2) == 2
        assert b"unknown processor %d" % processor in L.strsim_last_error_message()
    for measure in (5, 27, 28, 100, -1):
        assert f(ctx_stand_in, measure, 1, o, v, 2, o, v, 2, r, 2) == 2
        assert b"unknown measure %d" % measure in L.strsim_last_error_message()
    assert f(ctx_stand_in, 8, 1, o, v, 2, o, v, 3, r, 2) == 1
    assert L.strsim_last_error_message() == b"Inputs must have the same length, or one of them must be a Utf8 literal."
    assert f(ctx_stand_in, 8, 1, o, v, 2, o, v, 2, r, 3) == 2
    assert b"out_rows" in L.strsim_last_error_message()
    for args in ((None, v, o, v, r), (o, None, o, v, r), (o, v, None, v, r), (o, v, o, None, r), (o, v, o, v, None)):
        assert f(ctx_stand_in, 8, 1, args[0], args[1], 2, args[2], args[3], 2, args[4], 2) == 2
        assert b"NULL buffer" in L.strsim_last_error_message()
    for measure in (0, 2, 8, 10, 16, 26):
        assert f(None, measure, 1, o, v, 2, o, v, 2, r, 2) == 2   # every argument right: the NULL context, last
        assert b"ctx is NULL" in L.strsim_last_error_message()


# ---- the Python surfaces ----

def test_python_surface_without_a_device():
    import inspect

    import strsim_amd as S
    assert S.PROCESSORS == ("default_process",)
    assert S.__all__[:2] == ["default_process", "PROCESSORS"] and callable(S.default_process)
    for name in ("default_process_device", "default_process_host", "pairs_processed_device", "pairs_processed_host", "last_process_wave_rows"):
        assert hasattr(S.Context, name), name
    family = ("indel", "partial_ratio", "token_sort_ratio", "token_set_ratio", "token_ratio", "partial_token_sort_ratio",
              "partial_token_set_ratio", "partial_token_ratio", "wratio")
    for name in ("similarity", "extract") + family:
        p = list(inspect.signature(getattr(S, name)).parameters.values())[-1]
        assert p.name == "processor" and p.default is None, name
    for bad in ("lower", "", 1, b"default_process"):
        with pytest.raises(ValueError, match="unknown processor"):
            S.similarity("indel", ["a"], ["b"], processor=bad)
        with pytest.raises(ValueError, match="unknown processor"):
            S.wratio(["a"], ["b"], processor=bad)
        with pytest.raises(ValueError, match="unknown processor"):
            S.extract("ratio", ["a"], ["b"], processor=bad)


# ---- the plugin function as far as it goes without a device ----

@pytest.mark.parametrize("layout", ["vu", "u", "U"])
def test_plugin_zero_rows_field_and_release_without_a_device(layout):
    """Zero rows never reach a device: the whole export / import / release path of the plugin's first string result runs here."""
    import gc

    import pyarrow as pa
    from strsim_amd import arrow_host as H
    probe = {}
    got = H.call_plugin_unary("default_process", pa.array([], pa.string()), layout=layout, input_name="company", _probe=probe)
    assert got.type == pa.string() and got.to_pylist() == []
    assert probe["name"] == "company" and probe["format"] == "u"
    assert probe["series_released"] == [1] and probe["arrays_released"] == [True]
    assert probe["arrays_moved"] and probe["series_released_after"]
    del got
    gc.collect()  # (the array's release callback frees its buffers here)
    assert H.field_plugin("default_process", ("company",)) == ("company", pa.string())


def test_plugin_wrong_inputs_without_a_device():
    import pyarrow as pa
    from strsim_amd import arrow_host as H
    with pytest.raises(H.PluginError, match="expected `String`"):
        H.call_plugin_unary("default_process", pa.array([1, 2, 3], pa.int64()))
    with pytest.raises(H.PluginError, match="default_process: expected 1 input series, got 2"):
        H.call_plugin("default_process", ["a"], ["b"])
