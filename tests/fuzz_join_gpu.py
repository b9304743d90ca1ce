#!/usr/bin/env python3
"""Differential fuzz of the threshold join (strsim_join_*) against tests/join_ref.py: small random frames -- short alphabets so that
hits are common, duplicates, empty strings, strings outside the lane class (longer than 32 bytes, non-ASCII) on either side, token
frames for token_sort_ratio -- at random cutoffs, with and without `upper`: indptr, indices and scores bit for bit, and the count-only
call.  One pass over the frames, no retries.
Usage: python tests/fuzz_join_gpu.py [frames] [seed].  Exits non-zero on the first mismatch (prints the frame)."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the models are test infrastructure: this script lives in tests/
import numpy as np

import join_ref as R
import strsim_amd as S

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 150
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = random.Random(seed)
ALPHABETS = ("ab", "abc", "abcdefgh", "abcdefghijklmnopqrstuvwxyz", "aB _")
SLOW = ("é", "日本", "x" * 33, "abcabcabcabcabcabcabcabcabcabcabcabc", "ß" * 17)
CUTS = (None, 0.0, 0.3, 0.5, 2 / 3, 0.8, 0.9, 1.0, 1.5)


def string(alphabet, hi):
    r = rng.random()
    if r < 0.04:
        return rng.choice(SLOW) + "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 3)))
    return "".join(rng.choice(alphabet) for _ in range(rng.randint(0, hi)))


def column(alphabet, n, hi, pool):
    out = []
    for _ in range(n):
        if pool and rng.random() < 0.4:  # a copy, or a copy with an edit
            s = rng.choice(pool)
            if s and rng.random() < 0.5:
                p = rng.randrange(len(s))
                s = s[:p] + rng.choice(alphabet) + s[p + rng.randint(0, 1):]
            out.append(s)
        else:
            out.append(string(alphabet, hi))
    return out


ctx = S.Context(0)
pairs_total = hits_total = 0
for f in range(frames):
    alphabet = rng.choice(ALPHABETS)
    hi = rng.choice((3, 8, 16, 32))
    nq, nc = rng.choice((1, 2, 63, 64, 65, 130)), rng.choice((1, 5, 64, 129, 200))
    scorer = "token_sort_ratio" if rng.random() < 0.25 else "ratio"
    if scorer == "token_sort_ratio":
        alphabet = alphabet + "  "
    Cs = column(alphabet, nc, hi, [])
    Q = column(alphabet, nq, hi, Cs)
    upper = rng.random() < 0.4
    if upper and rng.random() < 0.5:
        Cs = Q  # a true self-join
    cut = rng.choice(CUTS)
    exp = R.join(scorer, Q, Cs, cut, upper)
    cols = (*S.pack_strings(Q), *S.pack_strings(Cs))
    got = ctx.join(R.MEASURE[scorer], *cols, cut, upper, capacity=rng.choice((None, 0, 1, int(exp[0][-1]))))
    counted = ctx.join(R.MEASURE[scorer], *cols, cut, upper, count_only=True)
    if not R.same(got, exp) or not np.array_equal(counted, exp[0]):
        print(f"MISMATCH frame {f} seed {seed}: {scorer} cutoff {cut!r} upper {upper}\nQ = {Q!r}\nC = {Cs!r}")
        print(f"gpu   {got[0].tolist()} {got[1].tolist()}\nmodel {exp[0].tolist()} {exp[1].tolist()}")
        sys.exit(1)
    pairs_total += len(Q) * len(Cs)
    hits_total += int(exp[0][-1])
print(f"fuzz_join ok: {frames} frames, {pairs_total} pairs, {hits_total} hits exact, seed {seed}")
