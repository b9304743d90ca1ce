#!/usr/bin/env python3
"""Differential fuzz of the Hamming / prefix / postfix / LCSseq calls (strsim_common_host, strsim_common_distance_host,
strsim_common_count_host) against tests/common_ref.py: random frames over small alphabets with lengths drawn around the boundaries
of the kernels (the dwords of the lane windows, the lane tier at 32 and LCSseq's at 128, the 64-byte chunks of the wave tier),
copies with substitutions, with another head or another tail, NUL bytes, 2- to 4-byte characters, a literal on either side now and
then; each frame through one kind's count (exactly), distance under a random cutoff (exactly) and similarity (bit for bit), with
the size of the second kernel's work list.
Usage: python tests/fuzz_common_gpu.py [frames] [seed].  Exits non-zero on the first mismatch (prints the row)."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the reference is test infrastructure: this script lives in tests/
import numpy as np

import common_ref as R
import strsim_amd as S

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 150
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = random.Random(seed)
ALPHABETS = ("a", "ab", "abc", "abcdefgh", "ab\0", "aé", "ab日😀", "é€😀", "".join(chr(c) for c in range(32, 128)))
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 30, 31, 32, 33, 34, 62, 63, 64, 65, 66, 127, 128, 129)
LONG = (254, 256, 258, 1023, 1025, 2047, 2049, 2300)


def length():
    r = rng.random()
    if r < 0.5:
        return rng.choice(LENGTHS)
    if r < 0.98:
        return rng.randint(0, 70)
    return rng.choice(LONG)


def string(alphabet, n=None):
    return "".join(rng.choice(alphabet) for _ in range(length() if n is None else n))


def row(alphabet):
    a = string(alphabet)
    r = rng.random()
    if r < 0.05:
        return a, a
    if r < 0.4:
        return a, R.edited(rng, a, alphabet, rng.randint(0, 3))
    if r < 0.55:  # another head: a common suffix, the lengths a few apart
        cut = rng.randint(0, len(a))
        return a, string(alphabet, rng.randint(0, 9)) + a[cut:]
    if r < 0.7:   # another tail: a common prefix
        cut = rng.randint(0, len(a))
        return a, a[:cut] + string(alphabet, rng.randint(0, 9))
    return a, string(alphabet)


def lane_row(kind, a, b):
    a, b = a.encode(), b.encode()
    cap = 128 if kind == "lcs_seq" else 32
    return len(a) <= cap and len(b) <= cap and max(a + b + b"\0") < 128


ctx = S.Context(0)
rows_total = 0
for f in range(frames):
    alphabet = rng.choice(ALPHABETS)
    kind = R.KINDS[f % 4]
    n = rng.choice((1, 2, 7, 63, 64, 65, 100, 130))
    A, B = (list(x) for x in zip(*(row(alphabet) for _ in range(n))))
    if rng.random() < 0.5:
        A, B = B, A
    lit = rng.random()
    if lit < 0.1:
        A = A[:1]
    elif lit < 0.2:
        B = B[:1]
    k = rng.choice((None, 0, 1, 2, 3, 10, 70))
    pa, pb = S.pack_strings(A), S.pack_strings(B)
    rows = max(len(A), len(B))
    AA, BB = (A * rows if len(A) == 1 else A), (B * rows if len(B) == 1 else B)
    slow = sum(not lane_row(kind, a, b) for a, b in zip(AA, BB))
    c, d, want = R.frame(kind, A, B)
    gc = ctx.common_count_host(kind, *pa, *pb)
    waves = [ctx.last_wave_rows]
    gd = ctx.common_distance_host(kind, *pa, *pb, k)
    waves.append(ctx.last_wave_rows)
    got = ctx.common_host(kind, *pa, *pb)
    waves.append(ctx.last_wave_rows)
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)) | (gd != R.clamp(d, k)) | (gc != c))
    if bad.size or waves != [slow] * 3:
        i = int(bad[0]) if bad.size else -1
        print(f"MISMATCH frame {f} {kind} k {k}: wave rows {waves} (expected {slow})"
              + (f", row {i}: {AA[i]!r} / {BB[i]!r} got {gc[i]} / {gd[i]} / {got[i]!r} want {c[i]} / d {d[i]} / {want[i]!r}" if bad.size else ""))
        sys.exit(1)
    rows_total += rows
print(f"fuzz_common ok: {frames} frames, {rows_total} rows exact, exact under a cutoff and bit-exact, seed {seed}")
