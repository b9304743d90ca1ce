#!/usr/bin/env python3
"""Differential fuzz of q-gram similarity (strsim_qgram_host) against tests/qgram_ref.py: random frames over small alphabets -- where
grams repeat -- with lengths drawn around the boundaries of the kernels (0 .. q + 1, the mask words at 32, the lane tier at 64, the
wave kernel's tables at 256 and 2 048 grams), NUL bytes, 2- to 4-byte characters, a literal on either side now and then; each
frame through the four kinds at one (q, mode), bit for bit, with the size of the second kernel's work list.
Usage: python tests/fuzz_qgram_gpu.py [frames] [seed].  Exits non-zero on the first mismatch (prints the row)."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the model is test infrastructure: this script lives in tests/
import numpy as np

import qgram_ref as R
import strsim_amd as S

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 150
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = random.Random(seed)
ALPHABETS = ("a", "ab", "abc", "abcdefgh", "ab\0", "aé", "ab日😀", "".join(chr(c) for c in range(32, 127)))
LENGTHS = (0, 1, 2, 3, 4, 5, 30, 31, 32, 33, 34, 62, 63, 64, 65, 66, 127, 128, 129)
LONG = (254, 256, 258, 1023, 1024, 1025, 1026, 2047, 2049, 3000)


def length():
    r = rng.random()
    if r < 0.55:
        return rng.choice(LENGTHS)
    if r < 0.97:
        return rng.randint(0, 70)
    return rng.choice(LONG)


def string(alphabet):
    return "".join(rng.choice(alphabet) for _ in range(length()))


def row(alphabet):
    a = string(alphabet)
    r = rng.random()
    if r < 0.1:
        return a, a
    if r < 0.4:  # an edited copy: many grams in common
        b = list(a)
        for _ in range(rng.randint(1, 3)):
            if b and rng.random() < 0.7:
                b[rng.randrange(len(b))] = rng.choice(alphabet)
            else:
                b.insert(rng.randint(0, len(b)), rng.choice(alphabet))
        return a, "".join(b)
    if r < 0.5 and a:  # a rotation: the same characters, other grams
        k = rng.randrange(len(a))
        return a, a[k:] + a[:k]
    return a, string(alphabet)


def lane_row(a, b):
    a, b = a.encode(), b.encode()
    return len(a) <= 64 and len(b) <= 64 and max(a + b + b"\0") < 128


ctx = S.Context(0)
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
    q, multiset = rng.choice((1, 2, 3)), rng.random() < 0.5
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    rows = max(len(A), len(B))
    AA, BB = (A * rows if len(A) == 1 else A), (B * rows if len(B) == 1 else B)
    slow = sum(not lane_row(a, b) for a, b in zip(AA, BB))
    for kind in R.KINDS:
        got = ctx.qgram_host(kind, ao, av, bo, bv, q, multiset)
        want = np.array(R.batch(kind, A, B, q, multiset), dtype=np.float64)
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        if bad.size or ctx.last_wave_rows != slow:
            i = int(bad[0]) if bad.size else -1
            print(f"MISMATCH frame {f} kind {kind} q {q} multiset {multiset}: wave rows {ctx.last_wave_rows} (expected {slow})"
                  + (f", row {i}: {AA[i]!r} / {BB[i]!r} got {got[i]!r} want {want[i]!r}" if bad.size else ""))
            sys.exit(1)
    rows_total += rows
print(f"fuzz_qgram ok: {frames} frames, {rows_total} rows x {len(R.KINDS)} kinds bit-exact, seed {seed}")
