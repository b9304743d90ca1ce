"""k_lane_stage<levenshtein> with register-table match masks in its long rounds (strsim_lane_ptab.h), bit for bit against the oracle.

A round of 64 length-sorted pairs takes the table core when its longest text (the shorter string of a pair) runs at least
STRSIM_STAGE_PTAB_MIN columns, rounded up to two; the frames put rounds on either side of that bound, on both in one block, on the
seven-plane path beside it, and in a partial block.  Frames are 4 096 rows (eight blocks of 512) through strsim_pairs_device.
"""
import os
import random
import re

import numpy as np
import pytest

import gen
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 4096


def _threshold():
    src = open(os.path.join(ROOT, "polars-strsim_amd", "csrc", "strsim_lane_stage.h")).read()
    return int(re.search(r"^#define STRSIM_STAGE_PTAB_MIN (\d+)", src, re.M).group(1))


@pytest.fixture(scope="module")
def S():
    import strsim_amd
    return strsim_amd


def _pairs(seed, n, lo, hi, alphabet=gen.ASCII_LOWER):
    """n pairs whose SHORTER string has lo .. hi bytes and whose longer one at most 32: an edited copy, a copy or an independent
    string, the longer one on either side."""
    rng = random.Random(seed)
    A, B = [], []
    while len(A) < n:
        s = gen.rand_string(rng, alphabet, lo, hi)
        r = rng.random()
        if r < 0.5:
            t = gen.edit(rng, s, alphabet, rng.randint(1, 3))
        elif r < 0.55:
            t = s
        else:
            t = gen.rand_string(rng, alphabet, len(s), 32)
        if len(t) > 32 or not lo <= min(len(s), len(t)) <= hi:
            continue
        if rng.random() < 0.5:
            s, t = t, s
        A.append(s)
        B.append(t)
    return A, B


def _run(S, A, B, expect_late=0):
    import torch
    oa, va = S.pack_strings(A)
    ob, vb = S.pack_strings(B)
    dev = torch.device("cuda", 0)
    t = lambda x, dt: torch.from_numpy(x.view(dt)).to(dev)
    pad = np.zeros(64, dtype=np.uint8)
    cols = (t(oa, np.int32), t(np.concatenate([va, pad]), np.uint8), t(ob, np.int32), t(np.concatenate([vb, pad]), np.uint8))
    torch.cuda.synchronize()
    exp = O.batch_strings("levenshtein", A, B, 8)
    with S.Context(0, one_launch=True) as ctx:
        before = ctx.enqueued_ops
        out = ctx.pairs_device("levenshtein", *cols)
        ops = ctx.enqueued_ops - before
        ctx.synchronize()
        late = ctx.last_late_rows
        got = out.cpu().numpy()
    bad = np.nonzero(got.view(np.uint64) != exp.view(np.uint64))[0]
    assert bad.size == 0, "%d / %d rows differ; first row %d: a=%r b=%r got=%r exp=%r" % (
        bad.size, len(A), bad[0], A[bad[0]], B[bad[0]], got[bad[0]], exp[bad[0]])
    # a fresh one-launch context enqueues the stage kernel alone; rows it flags in the mask are finished at retirement
    assert ops == 1
    if expect_late:
        assert late >= expect_late
    else:
        assert late == 0


def test_every_text_below_the_threshold(S):
    """(a) shorter strings of 1 .. T - 2 bytes: every round's bound stays below T, every round runs the bit fills."""
    T = _threshold()
    A, B = _pairs(11, ROWS, 1, min(T - 2, 32))
    _run(S, A, B)


def test_every_text_at_or_above_the_threshold(S):
    """(b) shorter strings of T - 1 .. 32 bytes (T - 1 rounds up to T): every round runs the table core, the longest all 32 columns."""
    T = _threshold()
    A, B = _pairs(12, ROWS, min(T - 1, 32), 32)
    _run(S, A, B)


def _uniform_frame(seed, n):
    rng = random.Random(seed)
    A = [gen.rand_string(rng, gen.ASCII_LOWER, 0, 32) for _ in range(n)]
    B = []
    for a in A:
        r = rng.random()
        b = gen.edit(rng, a, gen.ASCII_LOWER, rng.randint(1, 3)) if r < 0.5 else (a if r < 0.55 else gen.rand_string(rng, gen.ASCII_LOWER, 0, 32))
        B.append(b[:32])
    return A, B


def test_uniform_lengths_with_empty_strings(S):
    """(c) U{0..32} on both sides, empty strings included: the rounds of a block fall on both sides of the threshold."""
    A, B = _uniform_frame(13, ROWS)
    assert any(not a for a in A) and any(not b for b in B)
    A[5], B[5] = "", ""
    A[6], B[6] = "", "abc"
    A[7], B[7] = "abcdefghijklmnopqrstuvwxyzabcdef", ""
    _run(S, A, B)


def test_wide_rounds_and_non_ascii_rows_beside_the_table_rounds(S):
    """(d) frame (c) with digits and upper case in 1 row of 16 (their rounds take the seven-plane path) and 1 non-ASCII row in 64:
    that row's chunk is flagged in the mask and the row is finished by the later kernels, at retirement."""
    A, B = _uniform_frame(13, ROWS)
    rng = random.Random(14)
    wide = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    late = 0
    for i in range(ROWS):
        if i % 64 == 37:
            A[i] = ("é" + A[i])[:12]
            late += 1
        elif i % 16 == 3:
            A[i] = "".join(rng.choice(wide) if rng.random() < 0.4 else c for c in (A[i] or "x"))
            B[i] = "".join(rng.choice(wide) if rng.random() < 0.4 else c for c in B[i])
    _run(S, A, B, expect_late=late)


def test_partial_block_and_partial_round(S):
    """(e) 70 rows: one block that is not full, its last round six rows."""
    A, B = _uniform_frame(15, 70)
    A[0], B[0] = "abcdefghijklmnopqrstuvwxyzabcdef", "abcdefghijklmnopqrstuvwxyzabcdeg"  # (a 32-column round in it)
    _run(S, A, B)
