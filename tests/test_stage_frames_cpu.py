"""The frames of the block-cut tests keep their promises, by the plain-Python restatement of the cut (tests/stage_frames.py): no GPU.

The GPU tests (tests/test_stage_routes_gpu.py) import the same functions and assert the same before they call the device; here the
builders are checked over every case, and the restatement is checked against the three slips the frames exist to catch: each one
must change what the rule says about at least one frame, or the frame could not tell the kernels apart.
"""
import pytest

import stage_frames as F
import stage_routes as R

CAPS = [F.CAP_PLAIN, F.CAP_TABLES, F.CAP_LONG]
EDGE_CASES = [(d, delta, mis, base) for d in "ab" for delta in (-1, 0, 1) for mis in (0, 1, 15) for base in (0, 5)]


def test_routes_name_every_first_kernel():
    assert len(R.FIRST_KERNELS) == 17
    assert sum(k.startswith("k_lane_stage<") for k in R.FIRST_KERNELS) == 11
    assert sum(k.startswith("k_lane_lit<") for k in R.FIRST_KERNELS) == 5 and "k_lane_stage_all" in R.FIRST_KERNELS
    assert len({(R.route_id(r)) for r in R.ROUTES}) == len(R.ROUTES)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("decider,delta,mis,base", EDGE_CASES)
def test_edge_frame_keeps_its_promise(cap, decider, delta, mis, base):
    f = F.edge_frame(cap, decider, delta, mis, base)
    assert 1088 < len(f.A) == len(f.B) <= 1152 and f.shifts == (mis, mis) and f.bases == (base, base)
    blks = F.check_edge_frame(f, cap, "stage", decider, delta)
    # the next block starts from the carried base, with an alignment of its own
    assert blks[1].row0 == blks[0].rows and blks[1].mis[0] == (mis + base + sum(len(s) for s in f.A[:blks[0].rows])) % 16
    assert F.late_rows(blks, F.offsets(f.A, base), F.offsets(f.B, base)) == 0
    if cap == F.CAP_LIT:  # the literal kernel: the deciding column against a one-row side; its first workgroup has six chunks
        lit_side = "b" if decider == "a" else "a"
        assert F.ranges(len(f.A), "lit")[0] == (0, 6 * F.CHUNK)
        F.check_edge_frame(f, cap, "lit", decider, delta, literal_side=lit_side)


def test_edge_frames_are_reproducible_and_differ():
    a = F.edge_frame(F.CAP_PLAIN, "a", 0, 1, 5)
    F.edge_frame.cache_clear()
    b = F.edge_frame(F.CAP_PLAIN, "a", 0, 1, 5)
    assert a == b and a is not b
    assert F.edge_frame(F.CAP_PLAIN, "a", 0, 15, 0).A != F.edge_frame(F.CAP_PLAIN, "a", 1, 0, 0).A


def _cut_rows(name, cap, kind="stage", literal_side=None):
    return [b.rows for b in F.call_blocks(F.frame(name), cap, kind, literal_side)[0]]


@pytest.mark.parametrize("cap", CAPS)
def test_frame_b_is_cut_in_every_geometry(cap):
    """28..32-byte rows on both sides: no block of frame (b) reaches 512 rows, whichever staging size"""
    rows = _cut_rows("b", cap)
    assert sum(rows) == F.ROWS and max(rows) < F.BLOCK_ROWS
    assert max(_cut_rows("b", F.CAP_LIT, "lit", "b")) < F.BLOCK_ROWS


@pytest.mark.parametrize("cap", CAPS)
def test_frame_a_has_full_blocks_and_c_has_cuts_by_either_column(cap):
    assert set(_cut_rows("a", cap)) == {F.BLOCK_ROWS}
    f = F.frame("c")
    blks = F.call_blocks(f, cap, "stage")[0]
    cut = [b for b in blks if b.rows < F.BLOCK_ROWS and b.row0 + b.rows < len(f.A) and (b.row0 + b.rows) % 1024]
    # What frame (c) is at each staging size: 8 960 bytes: cuts of several lengths, either column the larger one; 10 240: cuts of
    # several lengths, all decided by column b (a window of 512 rows holds at most 312 long rows of column a); 15 104: no cut, a
    # column has at most 400 long rows in 512.  The edge frames put either column at the cut of every size.
    if cap == F.CAP_LONG:
        assert not cut
        return
    assert len({b.rows for b in cut}) >= 2
    assert {b.spans[0] > b.spans[1] for b in cut} == ({True, False} if cap == F.CAP_TABLES else {False})


@pytest.mark.parametrize("cap,kind,literal_side", [(c, "stage", s) for c in CAPS for s in (None, "b")] + [(F.CAP_LIT, "lit", "b"), (F.CAP_LIT, "lit", "a")])
def test_the_chunk_that_overflows_alone(cap, kind, literal_side):
    """(e) and its two variants: the rows the restated rule leaves to the later kernels"""
    at = 2048 + F.CHUNK
    assert F.call_late_rows(F.frame("e"), cap, kind, literal_side) == 64  # 200-byte rows, staged or not
    for name, late in (("e_long_first", 64), ("e_long_last", 48)):
        f = F.frame(name)
        blks = F.call_blocks(f, cap, kind, literal_side)[0]
        forced = [b for b in blks if b.row0 == at]
        assert len(forced) == 1 and forced[0].rows == F.CHUNK and min(s for s in forced[0].spans if s is not None) > cap
        assert [b.rows for b in blks if b.row0 == 2048] == [F.CHUNK]  # cut behind its first chunk
        assert F.call_late_rows(f, cap, kind, literal_side) == late


def test_primer_leaves_an_eighth_of_its_rows():
    f = F.frame("primer")
    assert len(f.A) == 1024 and sum(len(a) == 40 and a.isascii() for a in f.A) == 128
    for cap in CAPS:
        assert F.call_late_rows(f, cap, "stage") == 128


# ---- the slips the frames are for -------------------------------------------------------------------------------------------------------
def test_fit_test_off_by_one_changes_an_edge_frame():
    """`<=` -> `<` in the fit test: the frame whose span is exactly the cap loses its last chunk, in both kernels' rules"""
    strict = lambda span, cap: span < cap
    for cap, kind, lit in ((F.CAP_PLAIN, "stage", None), (F.CAP_TABLES, "stage", None), (F.CAP_LONG, "stage", None), (F.CAP_LIT, "lit", "b")):
        f = F.edge_frame(cap, "a", 0, 1, 5)
        right = F.call_blocks(f, cap, kind, lit)[0]
        wrong = F.call_blocks(f, cap, kind, lit, fit=strict)[0]
        assert right[0].chunks == F.edge_chunks(cap) and wrong[0].chunks == F.edge_chunks(cap) - 1
        with pytest.raises(AssertionError):
            F.check_edge_frame(f, cap, kind, "a", 0, literal_side=lit, fit=strict)


def test_the_window_behind_a_block_needs_the_32_bytes():
    """`+ 32u` dropped from chunksA: the window of a block's last row is 32 bytes from its first byte.  In an edge frame with
    delta = 0 the staged bytes are exactly the cap and the last row is shorter than 32 bytes, so its window reaches past them: the
    copy must take the bytes behind the block along, or the window shows the zero tail where the next block's text is."""
    for cap in CAPS:
        for delta in (-1, 0):
            f = F.edge_frame(cap, "a", delta, 0, 0)
            b0 = F.call_blocks(f, cap, "stage")[0][0]
            off = F.offsets(f.A)
            last = b0.row0 + b0.rows - 1
            assert b0.staged[0] == cap and off[last] + 32 > b0.staged[0] and off[-1] > b0.staged[0] + 32


def test_dma_iterations_of_the_long_geometry():
    """The copy of a block is cap + 32 bytes plus rounding in 16-byte pieces of 256 lanes: three iterations hold the plain and the
    table geometry, the long one needs four.  Frame (b) and the long edge frames have blocks beyond three iterations' bytes."""
    iters = lambda cap: -(-(cap + 48) // (16 * 256))
    assert [iters(c) for c in CAPS] == [3, 3, 4]
    beyond = 3 * 16 * 256
    assert max(max(b.staged) for b in F.call_blocks(F.frame("b"), F.CAP_LONG, "stage")[0]) > beyond
    assert F.call_blocks(F.edge_frame(F.CAP_LONG, "b", 0, 15, 5), F.CAP_LONG, "stage")[0][0].staged[1] > beyond
