"""Host-side check of the Levenshtein lane core with register-table match masks (strsim_lane_ptab.h).

lev_myers32_ptab<5> must return what lev_myers32_snap<5> returns and what the textbook DP returns, for every pair of lengths,
every column bound the kernel can hand it, and with the bytes behind both strings set to letters a leak would match.
"""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDIR = os.path.join(ROOT, "tests", "cpu_harness")
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")

ALPHABETS = {2: b"ab", 5: b"aeiou", 26: bytes(range(ord("a"), ord("z") + 1))}


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(HDIR, "liblane_core_ptab_harness.so")
    srcs = [os.path.join(HDIR, "lane_core_ptab_harness.cpp"), os.path.join(CSRC, "strsim_lane_core.h"),
            os.path.join(CSRC, "strsim_lane_ptab.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, srcs[0]])
    L = C.CDLL(so)
    L.harness_ptab_sweep.restype = C.c_int
    L.harness_ptab_sweep.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.harness_ptab_tables.restype = C.c_int
    L.harness_ptab_tables.argtypes = [C.c_char_p]
    return L


def _window(rng, alphabet, n, related=None):
    """A 32-byte window: a string of n letters, then letters of the same alphabet (what a neighbouring row would hold)."""
    if related is not None and rng.random() < 0.5:
        s = bytearray(related[:n])  # a near copy: small distances, long diagonal runs
        while len(s) < n:
            s.append(rng.choice(alphabet))
        for _ in range(rng.randint(0, 3)):
            s[rng.randrange(n)] = rng.choice(alphabet)
    else:
        s = bytearray(rng.choice(alphabet) for _ in range(n))
    return bytes(s) + bytes(rng.choice(alphabet) for _ in range(32 - n))


@pytest.mark.parametrize("letters", sorted(ALPHABETS))
def test_ptab_equals_snap_and_dp_for_every_length_pair_and_bound(harness, letters):
    """Every (lt, lp) with 1 <= lt <= lp <= 32; per pair every even tmax in [lt, 32] (so lt at the first and the last column of a
    four-column group, and tmax % 4 == 2) and every tmin in [1, lt]."""
    alphabet = ALPHABETS[letters]
    rng = random.Random(1000 + letters)
    out = (C.c_uint32 * 6)()
    runs = 0
    for lp in range(1, 33):
        for lt in range(1, lp + 1):
            wb = _window(rng, alphabet, lp)
            wa = _window(rng, alphabet, lt, related=wb)
            bad = harness.harness_ptab_sweep(wa, lt, wb, lp, out)
            assert bad == 0, dict(lt=lt, lp=lp, a=wa, b=wb, tmin=out[1], tmax=out[2], ptab=out[3], snap=out[4], dp=out[5])
            assert out[0] == lt * (17 - (lt + 1) // 2)
            runs += out[0]
    assert runs > 50000


def test_ptab_ignores_the_bytes_behind_both_strings(harness):
    """The same strings in front of different neighbours' bytes: every bound still gives the DP's distance of the strings alone
    (the harness compares with the DP over the first lt / lp bytes)."""
    rng = random.Random(7)
    out = (C.c_uint32 * 6)()
    alphabet = ALPHABETS[5]
    for lp in (1, 3, 4, 5, 8, 15, 16, 17, 24, 31, 32):
        for lt in sorted({1, 2, lp // 2 or 1, lp - 1 or 1, lp}):
            a = bytes(rng.choice(alphabet) for _ in range(lt))
            b = bytes(rng.choice(alphabet) for _ in range(lp))
            for tail in (a[-1:], b[-1:], b"a", b"u", b"z", b"\x7f", b"\x00"):
                wa, wb = a + tail * (32 - lt), b + tail * (32 - lp)
                assert harness.harness_ptab_sweep(wa, lt, wb, lp, out) == 0, (a, b, tail, list(out))
            wa, wb = a + b[:32 - lt].ljust(32 - lt, b"e"), b + a[:32 - lp].ljust(32 - lp, b"o")
            assert harness.harness_ptab_sweep(wa, lt, wb, lp, out) == 0, (a, b, list(out))


def test_ptab_tables_entry_by_entry(harness):
    """L[c & 7], M[c >> 3] from their byte slices, their AND, and ptab_masks against eq_mask<5> for all 32 five-bit characters."""
    rng = random.Random(3)
    for letters, alphabet in sorted(ALPHABETS.items()):
        for _ in range(200):
            assert harness.harness_ptab_tables(bytes(rng.choice(alphabet) for _ in range(32))) == 0
    for _ in range(500):  # any bytes: only the low five bits count
        assert harness.harness_ptab_tables(bytes(rng.randrange(256) for _ in range(32))) == 0
    for i in range(32):
        for c in range(32):
            w = bytearray(32)
            w[i] = c
            assert harness.harness_ptab_tables(bytes(w)) == 0
