#!/usr/bin/env python3
"""Differential fuzz of the unrestricted Damerau-Levenshtein calls (strsim_damerau_host, strsim_damerau_distance_host) against the
full-matrix DP of tests/damerau_ref.py (CRef): random frames over small alphabets -- where transpositions abound -- with lengths
drawn around the boundaries of the kernels (the lane tier at 32, the strips at 64 and 128, the boundary row's LDS sizes at 256 and
2 048), gapped and swapped copies, NUL bytes, 2- to 4-byte characters, a literal on either side now and then; each frame through
the similarity (bit for bit) and the distance under a random cutoff, with the size of the second kernel's work list.
Usage: python tests/fuzz_damerau_gpu.py [frames] [seed].  Exits non-zero on the first mismatch (prints the row)."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the reference is test infrastructure: this script lives in tests/
import numpy as np

import damerau_ref as R
import strsim_amd as S

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 150
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = random.Random(seed)
ALPHABETS = ("a", "ab", "abc", "abcdefgh", "ab\0", "aé", "ab日😀", "".join(chr(c) for c in range(32, 127)))
LENGTHS = (0, 1, 2, 3, 30, 31, 32, 33, 34, 62, 63, 64, 65, 66, 127, 128, 129)
LONG = (254, 256, 258, 1023, 1025, 2047, 2048, 2049, 2300)


def length():
    r = rng.random()
    if r < 0.5:
        return rng.choice(LENGTHS)
    if r < 0.98:
        return rng.randint(0, 70)
    return rng.choice(LONG)


def string(alphabet):
    return "".join(rng.choice(alphabet) for _ in range(length()))


def row(alphabet):
    a = string(alphabet)
    r = rng.random()
    if r < 0.05:
        return a, a
    if r < 0.4:
        return a, R.gapped(rng, a, rng.randint(1, 3), alphabet)
    if r < 0.6:
        return a, R.swapped(rng, R.gapped(rng, a, 1, alphabet), rng.randint(1, 3))
    if r < 0.7:
        return R.gapped(rng, a, 2, alphabet), a[:rng.randint(0, len(a))]
    return a, string(alphabet)


def lane_row(a, b):
    a, b = a.encode(), b.encode()
    return len(a) <= 32 and len(b) <= 32 and max(a + b + b"\0") < 128


ctx = S.Context(0)
cref = R.CRef()
rows_total = 0
for f in range(frames):
    alphabet = rng.choice(ALPHABETS)
    n = rng.choice((1, 2, 7, 63, 64, 65, 100, 130, 300))
    A, B = (list(x) for x in zip(*(row(alphabet) for _ in range(n))))
    lit = rng.random()
    if lit < 0.1:
        A = A[:1]
    elif lit < 0.2:
        B = B[:1]
    k = rng.choice((None, 0, 1, 2, 3, 10, 70))
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    rows = max(len(A), len(B))
    AA, BB = (A * rows if len(A) == 1 else A), (B * rows if len(B) == 1 else B)
    slow = sum(not lane_row(a, b) for a, b in zip(AA, BB))
    d = cref.distances(A, B)
    want = cref.scores(A, B)
    got = ctx.damerau_host(ao, av, bo, bv)
    wave_sim = ctx.last_wave_rows
    gd = ctx.damerau_distance_host(ao, av, bo, bv, k)
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)) | (gd != R.clamp(d, k)))
    if bad.size or wave_sim != slow or ctx.last_wave_rows != slow:
        i = int(bad[0]) if bad.size else -1
        print(f"MISMATCH frame {f} k {k}: wave rows {wave_sim} / {ctx.last_wave_rows} (expected {slow})"
              + (f", row {i}: {AA[i]!r} / {BB[i]!r} got {got[i]!r} / {gd[i]} want {want[i]!r} / d {d[i]}" if bad.size else ""))
        sys.exit(1)
    rows_total += rows
print(f"fuzz_damerau ok: {frames} frames, {rows_total} rows bit-exact and exact under a cutoff, seed {seed}")
