"""k_lane_stage<levenshtein>: the block cut, the store phase behind it and the instantiation without literal code, bit for bit
against the oracle.

A workgroup takes ranges of at least two blocks of up to 512 rows; a block is cut to the 64-row chunks whose bytes fit the staging
area of 10 240 bytes per column.  A block's base offsets are the previous block's end offsets while the range lasts, so the frames
put full blocks, cut blocks, cuts of changing length, a forced one-chunk block and one-row and
one-chunk last blocks behind one another.  Frames are a few thousand rows through strsim_pairs_device on a fresh one-launch context.

These are the Levenshtein cases the frames were first built for: k_lane_stage<levenshtein, 0, 0, 1>, its literal-keeping sibling
and k_lane_lit<levenshtein>.  The frames themselves live in tests/stage_frames.py, built once and shared;
tests/test_stage_routes_gpu.py runs them, and the frames whose block fits its staging area exactly or misses it by a byte, over
every first kernel of a pairwise call (tests/stage_routes.py: 17 kernels, four staging sizes, three geometries).

The column-only instantiation is a compile-time knob of strsim_lane_stage.h (STRSIM_STAGE_COLS_ONLY) that ships on; the results do
not depend on it.  (The frames were built when the cut could also carry its offsets from block to block and the store phase could
be split around it: LAB_NOTES 3.1c, 3.1d.)
"""
import numpy as np
import pytest

import oracle_lib as O
import stage_frames as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import strsim_amd
    return strsim_amd


def _uniform():
    """frame (a): U{0..32} on both sides, 4 096 rows, with its expected results (shared, never changed)"""
    f = F.frame("a")
    return f.A, f.B, F.expected("a", "levenshtein")


def _column(S, strings, dev, shift=0):
    """(offsets, values) on the device; the value buffer starts `shift` bytes behind a 16-byte boundary, 64 readable bytes follow it"""
    import torch
    off, val = S.pack_strings(list(strings))
    buf = np.concatenate([np.full(shift, 0xE9, dtype=np.uint8), val.view(np.uint8), np.zeros(64, dtype=np.uint8)])
    values = torch.from_numpy(buf).to(dev)[shift:]
    assert values.data_ptr() % 16 == shift % 16
    return torch.from_numpy(off.view(np.int32)).to(dev), values


def _run(S, A, B, exp=None, late=0, shifts=(0, 0), one_op=True):
    import torch
    dev = torch.device("cuda", 0)
    cols = _column(S, A, dev, shifts[0]) + _column(S, B, dev, shifts[1])
    torch.cuda.synchronize()
    n = max(len(A), len(B))
    if exp is None:
        exp = O.batch_strings("levenshtein", list(A) * (n if len(A) == 1 else 1), list(B) * (n if len(B) == 1 else 1), 8)
    with S.Context(0, one_launch=True) as ctx:
        before = ctx.enqueued_ops
        out = ctx.pairs_device("levenshtein", *cols)
        ops = ctx.enqueued_ops - before
        ctx.synchronize()
        got_late = ctx.last_late_rows
        got = out.cpu().numpy()
    bad = np.nonzero(got.view(np.uint64) != exp.view(np.uint64))[0]
    assert bad.size == 0, "%d / %d rows differ; first row %d: a=%r b=%r got=%r exp=%r" % (
        bad.size, n, bad[0], A[bad[0] % len(A)], B[bad[0] % len(B)], got[bad[0]], exp[bad[0]])
    if one_op:
        assert ops == 1  # a fresh one-launch context enqueues the stage kernel alone; flagged rows are finished at retirement
    assert got_late == late


def test_full_blocks(S):
    """(a) full blocks of 512 rows: the base carried behind a full block, re-read at the start of a range."""
    A, B, exp = _uniform()
    _run(S, A, B, exp)


def test_every_block_cut(S):
    """(b) every string 28..32 bytes: 512 rows overflow the staging area, every block is cut to about five chunks; the carried base is
    the cut block's end, not the end of the rows whose offsets were loaded."""
    f = F.frame("b")
    _run(S, f.A, f.B, F.expected("b", "levenshtein"))


def test_cuts_of_changing_length(S):
    """(c) runs of 200 rows of 30..32-byte strings and of 0..4-byte strings: cuts of different lengths follow one another inside a
    range, and in half of the runs column a is long where column b is short.  (At 10 240 bytes column b decides every cut of this
    frame, at 8 960 either column does: tests/test_stage_frames_cpu.py.  The edge frames put either column at every cut.)"""
    f = F.frame("c")
    _run(S, f.A, f.B, F.expected("c", "levenshtein"))


@pytest.mark.parametrize("n", [70, 1024 + 1, 1088])
def test_small_frames(S, n):
    """(d) one block that is not full; a one-row last block at the start of a range; a last block of a single chunk."""
    f = F.frame("d%d" % n)
    _run(S, f.A, f.B, F.expected(f.name, "levenshtein"))


def test_one_chunk_overflows_alone(S):
    """(e) 64 rows of 200-byte strings inside frame (a), one chunk behind the start of a block: that block is cut behind its first
    chunk, the next one is the chunk that overflows alone (at least one chunk is taken), the one behind it starts from the forced
    block's end.  The 64 rows are longer than 32 bytes: the later kernels finish them."""
    f = F.frame("e")
    _run(S, f.A, f.B, F.expected("e", "levenshtein"), late=64)


LITERALS = F.LITERALS


@pytest.mark.parametrize("stage_kernel", [True, False])
@pytest.mark.parametrize("side", ["a", "b"])
def test_literal_on_either_side(S, monkeypatch, side, stage_kernel):
    """(f) a one-row side against frame (a)'s other column: an empty literal, a 32-byte one and a short one.  With
    STRSIM_NO_LITERAL_PATH the call takes the stage kernel's instantiation that keeps the literal's code; without it the literal
    kernel, which this change does not touch."""
    if stage_kernel:
        monkeypatch.setenv("STRSIM_NO_LITERAL_PATH", "1")
    else:
        monkeypatch.delenv("STRSIM_NO_LITERAL_PATH", raising=False)
    A, B, _ = _uniform()
    for lit in LITERALS:
        exp = F.expected("a", "levenshtein", side, lit)
        if side == "a":
            _run(S, [lit], B, exp, one_op=stage_kernel)
        else:
            _run(S, A, [lit], exp, one_op=stage_kernel)


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_misaligned_value_buffers(S, shift):
    """(g) frame (a) with the value buffers 1, 7 and 15 bytes behind a 16-byte boundary (column b: 15, 9 and 1): the alignment of a
    block's copy derives from a carried base."""
    A, B, exp = _uniform()
    _run(S, A, B, exp, shifts=(shift, 16 - shift))
