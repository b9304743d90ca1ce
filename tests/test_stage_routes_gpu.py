"""Every first kernel of a pairwise call at its block cut, bit for bit against the oracle: the frames of tests/stage_frames.py over
the routes of tests/stage_routes.py.

  frames   the full blocks, the cut blocks, the cuts of changing length, the small frames, the chunk that overflows alone (and its
           two variants with lane-class rows outside the staged bytes) and the misaligned value buffers, on every route;
  edges    frames whose first block has a span of cap - 1, cap and cap + 1 bytes, by either column, at three alignments of the
           value buffer and two bases, on every route whose staging size they were built for;
  switch   one context that changes between the short-row and the long-row geometry from call to call.

Before a frame goes to the device the test asserts, by the plain-Python restatement of the cut, that the frame does what it is
for.  Where a call enqueues the first kernel alone, last_late_rows is that kernel's count of the rows it left, and it must equal
what the restatement leaves; on the long route the later kernels run in stream order and the counter stays 0.

Every frame is valid UTF-8 (ASCII) with 64 readable bytes behind each value buffer.
"""
import numpy as np
import pytest

import stage_frames as F
import stage_routes as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import strsim_amd
    return strsim_amd


def _device_column(strings, dev, shift=0, base=0):
    """(offsets, values) on the device: the value buffer starts `shift` bytes behind a 16-byte boundary, offsets[0] == base"""
    import torch
    off, buf = F.column_bytes(strings, shift, base)
    values = torch.from_numpy(buf).to(dev)[shift:]
    assert values.data_ptr() % 16 == shift % 16 and int(off[0]) == base
    return torch.from_numpy(off.view(np.int32)).to(dev), values


def _frame_columns(f, literal_side=None, literal=F.LITERAL):
    import torch
    dev = torch.device("cuda", 0)
    A, B = F.sides(f, literal_side, literal)
    ca = _device_column(A, dev) if literal_side == "a" else _device_column(A, dev, f.shifts[0], f.bases[0])
    cb = _device_column(B, dev) if literal_side == "b" else _device_column(B, dev, f.shifts[1], f.bases[1])
    torch.cuda.synchronize()
    return ca + cb


def _enqueue(ctx, measure, cols):
    """-> (outputs, measures, operations enqueued)"""
    before = ctx.enqueued_ops
    if measure == R.ALL:
        outs, measures = ctx.pairs_device_all(*cols), R.MEASURES
    else:
        outs, measures = [ctx.pairs_device(measure, *cols)], (measure,)
    return outs, measures, ctx.enqueued_ops - before


def _compare(f, outs, measures, literal_side=None, literal=F.LITERAL):
    A, B = F.sides(f, literal_side, literal)
    for out, m in zip(outs, measures):
        got, exp = out.cpu().numpy(), F.expected(f.name, m, literal_side, literal)
        bad = np.nonzero(got.view(np.uint64) != exp.view(np.uint64))[0]
        assert bad.size == 0, "%s %s: %d / %d rows differ; first row %d: a=%r b=%r got=%r exp=%r" % (
            f.name, m, bad.size, exp.size, bad[0], A[bad[0] % len(A)], B[bad[0] % len(B)], got[bad[0]], exp[bad[0]])


def _prime(ctx):
    """A call that leaves more than 1/16 of its rows behind the first kernel, on a context that expects no slow rows: the next call
    on ctx takes the long-row geometry (strsim_capi.cpp, ctx_retire_slot: c->long_rows = left * 16 > n)"""
    f = F.frame("primer")
    outs, measures, ops = _enqueue(ctx, "levenshtein", _frame_columns(f))
    ctx.synchronize()
    assert ops == 1                                # the call was deferred, so the counter is the kernel's lane_left
    assert ctx.last_late_rows * 16 > len(f.A)
    _compare(f, outs, measures)


def _call(S, monkeypatch, route, f, literal_side=None, literal=F.LITERAL):
    """one call of frame f on the route, on a context of its own; -> last_late_rows of the call"""
    monkeypatch.delenv("STRSIM_NO_LITERAL_PATH", raising=False)
    for k, v in route.env.items():
        monkeypatch.setenv(k, v)
    cols = _frame_columns(f, literal_side, literal)
    with S.Context(0, one_launch=True) as ctx:
        if route.primed:
            _prime(ctx)
        outs, measures, ops = _enqueue(ctx, route.measure, cols)
        ctx.synchronize()
        late = ctx.last_late_rows
        _compare(f, outs, measures, literal_side, literal)
    # (the five-output pass on a primed context would be 1 + 21; it has no long route)
    assert ops == route.ops, "%s enqueued %d operations, not %d: the call did not take the route" % (R.route_id(route), ops, route.ops)
    return late


def _expect_late(route, f, literal_side, literal=F.LITERAL):
    # a primed context's call is not deferred: nothing is finished late, nothing is counted
    return 0 if route.primed else F.call_late_rows(f, route.cap, route.kind, literal_side, literal)


@pytest.mark.parametrize("name", F.FRAME_NAMES)
@pytest.mark.parametrize("route", R.ROUTES, ids=R.route_id)
def test_frames(S, monkeypatch, route, name):
    f = F.frame(name)
    for side in route.sides:
        blks = F.call_blocks(f, route.cap, route.kind, side)[0]
        if name == "a" or name.startswith("g"):
            assert {b.rows for b in blks} == {F.BLOCK_ROWS}
        elif name == "b":  # cut in every geometry
            assert max(b.rows for b in blks) < F.BLOCK_ROWS
        elif name.startswith("e_"):  # the chunk overflows this route's staging area alone
            forced = [b for b in blks if b.row0 == 2048 + F.CHUNK]
            assert forced[0].rows == F.CHUNK and min(s for s in forced[0].spans if s is not None) > route.cap
        assert _call(S, monkeypatch, route, f, side) == _expect_late(route, f, side)
        if name == "a" and side is not None:  # an empty one-row side and one of 32 bytes
            for lit in F.LITERALS[:2]:
                assert _call(S, monkeypatch, route, f, side, lit) == 0


def _literal_side(route, decider):
    """the side of the one-row string: it stands against the deciding column"""
    return None if route.sides == (None,) else ("b" if decider == "a" else "a")


# (the five-output pass has its one-row side on b only: column a decides)
EDGE_ROUTES = [(r, d) for r in R.ROUTES for d in "ab" if _literal_side(r, d) in r.sides]


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("route,decider", EDGE_ROUTES, ids=lambda v: v if isinstance(v, str) else R.route_id(v))
def test_edges(S, monkeypatch, route, decider, delta):
    side = _literal_side(route, decider)
    for mis in (0, 1, 15):
        for base in (0, 5):
            f = F.edge_frame(route.cap, decider, delta, mis, base)
            F.check_edge_frame(f, route.cap, route.kind, decider, delta, literal_side=side)
            assert _call(S, monkeypatch, route, f, side) == 0


@pytest.mark.parametrize("measure", R.MEASURES)
def test_geometry_switch(S, monkeypatch, measure):
    """One one-launch context: primer | frame (b), frame (a) | frame (a) | primer | an edge frame, retired at each `|`.

    What the next call is enqueued for is decided when a call is RETIRED (ctx_retire_slot: expect_slow = left != 0, long_rows =
    left * 16 > n), so: the primer runs alone on the fresh context (1 operation) and leaves 128 of 1 024 rows; (b) and the first
    (a), enqueued behind it before either is retired, both take the long-row geometry with the later kernels behind them (5 and
    5); both leave nothing, so the second (a) and the second primer run alone in the short-row geometry (1 and 1); the edge frame
    behind the primer is the long geometry's again (5)."""
    monkeypatch.delenv("STRSIM_NO_LITERAL_PATH", raising=False)
    edge = F.edge_frame(F.CAP_LONG, "a", 0, 1, 5)
    F.check_edge_frame(edge, F.CAP_LONG, "stage", "a", 0)
    steps = [("primer", True), ("b", False), ("a", True), ("a", True), ("primer", True), (edge.name, True)]
    ops, late, pending = [], [], []
    with S.Context(0, one_launch=True) as ctx:
        for name, retire in steps:
            f = F.frame(name)
            outs, measures, n_ops = _enqueue(ctx, measure, _frame_columns(f))
            ops.append(n_ops)
            pending.append((f, outs, measures))
            if retire:
                ctx.synchronize()
                late.append(ctx.last_late_rows)
                for p in pending:
                    _compare(*p)
                pending = []
    assert ops == [1, 5, 5, 1, 1, 5], ops
    assert late == [128, 0, 0, 128, 0], late
