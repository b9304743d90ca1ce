#!/usr/bin/env python3
"""Differential fuzz of token_ratio, the partial token ratios and wratio (ids 18 .. 26) against tests/wratio_ref.py: random frames of
small rows -- token vocabularies, duplicates, every whitespace class, non-ASCII tokens, empty rows, length ratios around 1.5 and 8,
a literal on either side now and then -- each through all five measures, bit for bit, with the routing counts of wratio.
Usage: python tests/fuzz_wratio_gpu.py [frames] [seed].  Exits non-zero on the first mismatch (prints the row)."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the models are test infrastructure: this script lives in tests/
import numpy as np

import strsim_amd as S
import wratio_ref as W

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 300
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = random.Random(seed)
VOCABS = (("ab", "abc", "b"), ("a", "b", "c", "d", "e"), ("new", "york", "mets", "yankees", "the"), ("é", "äb", "漢字", "ab", "ß"),
          tuple("".join(chr(97 + (i * j) % 7) for j in range(1, 2 + i % 5)) for i in range(1, 40)))
SPACES = (" ", "  ", "\t", " ", "　", "  ", "\n")
NAMES = S.WEIGHTED_MEASURES


def string(vocab, n_tokens):
    s = "".join(rng.choice(vocab) + rng.choice(SPACES if rng.random() < 0.15 else (" ",)) for _ in range(n_tokens))
    r = rng.random()
    return s if r < 0.1 else (" " + s if r < 0.2 else s.rstrip())


def row(vocab):
    r = rng.random()
    if r < 0.03:
        return rng.choice(("", " ", "\t ")), string(vocab, rng.randint(0, 3))
    a = string(vocab, rng.randint(1, 4))
    if r < 0.45:  # near: a shuffled copy with an edit now and then
        t = a.split()
        rng.shuffle(t)
        if rng.random() < 0.5 and t:
            t[rng.randrange(len(t))] = rng.choice(vocab)
        return a, " ".join(t)
    if r < 0.75:  # far: a inside something longer
        return a, string(vocab, rng.randint(2, 6)) + a + " " + string(vocab, rng.randint(2, 12))
    return a, string(vocab, rng.randint(1, 14))


model = W.Frames()
ctx = S.Context(0)
rows_total = 0
for f in range(frames):
    vocab = rng.choice(VOCABS)
    n = rng.choice((1, 2, 7, 63, 64, 65, 100, 130))
    A, B = (list(x) for x in zip(*(row(vocab) for _ in range(n))))
    if rng.random() < 0.5:
        A, B = B, A
    lit = rng.random()
    if lit < 0.1:
        A = A[:1]
    elif lit < 0.2:
        B = B[:1]
    cols = model.columns(A, B)
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    for name in NAMES:
        got = ctx.pairs_host(name, ao, av, bo, bv)
        bad = np.flatnonzero(got.view(np.uint64) != cols[name].view(np.uint64))
        if bad.size:
            i = int(bad[0])
            X, Y = W.T.broadcast(A, B)
            print(f"MISMATCH frame {f} seed {seed} {name} row {i}: {X[i]!r} / {Y[i]!r}: gpu {got[i]!r} model {cols[name][i]!r}")
            sys.exit(1)
    want = (int((cols["class"] == W.NEAR).sum()), int((cols["class"] >= W.FAR8).sum()))
    if ctx.last_wratio_rows() != want:
        print(f"MISMATCH frame {f} seed {seed}: routed {ctx.last_wratio_rows()}, the model routes {want}")
        sys.exit(1)
    rows_total += len(cols["class"])
print(f"fuzz_wratio ok: {frames} frames, {rows_total} rows x {len(NAMES)} measures bit-exact, seed {seed}")
