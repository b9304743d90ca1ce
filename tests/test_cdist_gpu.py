"""cdist on the MI355X (strsim_cdist_*) against the contract stated independently (tests/cdist_ref.py): the score of every pair
from the models the searches are tested against, then the cutoff rule.  Every comparison is on uint64 views: bit for bit."""
import functools
import math
import random

import numpy as np
import pytest

import best_match_ref
import cdist_ref as R
import gen
import indel_ref
import token_ref

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")
MEASURES = R.MEASURES
INF = float("inf")
TJ = 8  # CDIST_TJ of strsim_cdist.h; the widths below also straddle a tile of 16
SENTINEL = 0x7FF8C0FFEE15BAD1  # a NaN payload no score has


def E(d, s):
    return indel_ref.normalise(d, s, 0)


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def _run(ctx, measure, Q, Cs, cut=None):
    qo, qv = S.pack_strings(Q)
    co, cv = S.pack_strings(Cs)
    out = ctx.cdist(R.MEASURE[measure], qo, qv, co, cv, cut)
    assert out.shape == (len(Q), len(Cs)) and out.dtype == np.float64
    return out


def _assert_same(got, exp, what=""):
    assert got.shape == exp.shape
    bad = np.argwhere(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(exp).view(np.uint64))
    assert bad.size == 0, "%s: %d of %d elements differ, first (%d, %d): got %r, expected %r" % (
        what, len(bad), got.size, bad[0][0], bad[0][1], got[tuple(bad[0])], exp[tuple(bad[0])])


def _strings(seed, n, alphabet=gen.ASCII_LOWER, lo=0, hi=12):
    A, B = gen.pairs(seed, (n + 1) // 2, alphabet, lo, hi)
    return (A + B)[:n]


def _frame(measure, seed, n, **kw):
    """strings of 0..12 characters; for token_sort_ratio some letters become spaces: tokens to sort"""
    X = _strings(seed, n, **kw)
    return [s.replace("e", " ").replace("t", " ") for s in X] if measure == "token_sort_ratio" else X


def _device_columns(torch, *cols):
    dev = torch.device("cuda", 0)
    out = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.uint8)).to(dev) for x in cols]
    torch.cuda.synchronize()
    return out


# ---- the tile's edges ---------------------------------------------------------------------------------------------------------

Q_EDGES = (1, 63, 64, 65, 257, 513)
C_EDGES = (1, TJ - 1, TJ, TJ + 1, 2 * TJ + 3, 15, 16, 17, 2 * 16 + 3)


@functools.lru_cache(maxsize=None)
def _edge_frame(measure):
    Q = _frame(measure, 101, max(Q_EDGES))
    Cs = _frame(measure, 102, max(C_EDGES))
    M = R.score_matrix(measure, Q, Cs)
    M.setflags(write=False)
    return Q, Cs, M


@pytest.mark.parametrize("measure", MEASURES)
def test_cdist_gpu_tile_edges(ctx, measure):
    # one query wave less a lane, exactly one, one more, and more than a workgroup; candidates around one and two tiles
    Q, Cs, M = _edge_frame(measure)
    for q in Q_EDGES:
        for c in C_EDGES:
            _assert_same(_run(ctx, measure, Q[:q], Cs[:c]), M[:q, :c], "%s %d x %d" % (measure, q, c))


@pytest.mark.parametrize("measure", ["levenshtein", "ratio"])
@pytest.mark.parametrize("c", [4 * TJ + 2, 4 * TJ + 3])
@pytest.mark.parametrize("shift", [0, 1])
def test_cdist_gpu_padded_rows_and_a_misaligned_base(ctx, measure, c, shift):
    # ld = c + 3 (odd and even: the 16-byte phase of a row alternates or not), out at a 16-byte boundary and 8 bytes past one; the
    # padding of every row and the words around the matrix hold a sentinel that must survive
    torch = pytest.importorskip("torch")
    Q, Cs, M = _edge_frame(measure)
    q, ld = 65, c + 3
    cols = _device_columns(torch, *S.pack_strings(Q[:q]), *S.pack_strings(Cs[:c]))
    flat = torch.from_numpy(np.full(4 + q * ld + 4, SENTINEL, dtype=np.uint64).view(np.int64)).to(cols[0].device).view(torch.float64)
    assert flat.data_ptr() % 16 == 0
    first = 2 + shift
    out = flat.as_strided((q, c), (ld, 1), first)
    assert out.data_ptr() % 16 == 8 * shift
    ctx.cdist(R.MEASURE[measure], *cols, out=out)
    ctx.synchronize()
    raw = flat.view(torch.int64).cpu().numpy().view(np.uint64)
    body = raw[first:first + q * ld].reshape(q, ld)
    _assert_same(body[:, :c].view(np.float64), M[:q, :c], "%s ld %d shift %d" % (measure, ld, shift))
    assert (body[:, c:] == SENTINEL).all() and (raw[:first] == SENTINEL).all() and (raw[first + q * ld:] == SENTINEL).all()


@functools.lru_cache(maxsize=None)
def _split_frames(measure):
    out = []
    for seed, q, c in ((111, 5, 3000), (113, 300, 700)):
        Q, Cs = _frame(measure, seed, q), _frame(measure, seed + 1, c)
        out.append((Q, Cs, R.score_matrix(measure, Q, Cs)))
    return out


@pytest.mark.parametrize("measure", MEASURES)
def test_cdist_gpu_several_splits(ctx, measure):
    # few query workgroups: the candidates are split over grid.y, and a split's last tile is cut short
    for Q, Cs, M in _split_frames(measure):
        _assert_same(_run(ctx, measure, Q, Cs), M, "%s %d x %d" % (measure, len(Q), len(Cs)))


@pytest.mark.parametrize("measure", MEASURES)
def test_cdist_gpu_five_and_seven_plane_waves(ctx, measure):
    # a wave of lower-case queries runs five planes against lower-case candidates and seven against mixed ones
    Q = _strings(121, 128) + _strings(122, 70, alphabet="abcXYZ09 -.,")
    Cs = _strings(123, 40) + _strings(124, 30, alphabet="aBcXyZ09_ !") + ["HELLO", "hello", "Hello"]
    _assert_same(_run(ctx, measure, Q, Cs), R.score_matrix(measure, Q, Cs), measure)


@pytest.mark.parametrize("measure", MEASURES)
def test_cdist_gpu_empty_strings(ctx, measure):
    Q = ["", "a", "", "abc", ""]
    Cs = ["", "abc", "", "b"]
    M = R.score_matrix(measure, Q, Cs)
    _assert_same(_run(ctx, measure, Q, Cs), M, measure)
    assert M[0, 0] == 1.0 and M[0, 1] == 0.0
    _assert_same(_run(ctx, measure, [""] * 3, ["", ""]), np.ones((3, 2)), measure)
    _assert_same(_run(ctx, measure, ["", "x"], ["abc"]), R.score_matrix(measure, ["", "x"], ["abc"]), measure)
    assert _run(ctx, measure, [], ["a"]).shape == (0, 1) and _run(ctx, measure, ["a"], []).shape == (1, 0)


# ---- strings outside the lane class -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("side", ["query", "candidate", "both"])
@pytest.mark.parametrize("cut", [None, 0.4])
def test_cdist_gpu_slow_strings(ctx, measure, side, cut):
    # a 33-byte ASCII query and a 2-byte-UTF-8 candidate go through the pairwise call: their row and column are exact and the
    # rows and columns around them are undisturbed (the whole matrix is compared)
    Q = _frame(measure, 131, 70)
    Cs = _frame(measure, 132, 37)
    if side in ("query", "both"):
        Q[33] = "abcdefghij klmnopqrst uvwxyzabcde"[:33]
        assert len(Q[33].encode()) == 33
    if side in ("candidate", "both"):
        Cs[17] = "héllo wörld"
    if side == "both":
        Q[64] = "ñandú"
        Cs[0] = "x" * 40
    _assert_same(_run(ctx, measure, Q, Cs, cut), R.cdist(measure, Q, Cs, cut), "%s %s" % (measure, side))


@functools.lru_cache(maxsize=None)
def _batch_boundary_frame(measure, side):
    Q, Cs = gen.batch_boundary_frame(161, side)
    M = R.score_matrix(measure, Q, Cs)
    M.setflags(write=False)
    return Q, Cs, M


@pytest.mark.parametrize("side", ["queries", "candidates", "both"])
@pytest.mark.parametrize("cut", ["zero", "between"])
def test_cdist_gpu_more_slow_strings_than_one_batch(ctx, side, cut):
    # 37 slow queries and 21 slow candidates (gen.batch_boundary_frame): the fallback walks three batches of rows and two of
    # columns, so the row cutoff and the column scatter run on a batch that is not the first.  "between": a cutoff strictly
    # between two attained scores, so the pairs at the lower one are zeroed and those at the upper one are kept.
    for measure in MEASURES:
        Q, Cs, M = _batch_boundary_frame(measure, side)
        c = 0.0
        if cut == "between":
            v = np.unique(M)
            lo, hi = float(v[len(v) // 2 - 1]), float(v[len(v) // 2])
            c = (lo + hi) / 2
            assert lo < c < hi
        exp = R.apply_cutoff(M, c)
        assert cut == "zero" or ((exp == 0.0) & (M != 0.0)).any()
        _assert_same(_run(ctx, measure, Q, Cs, c), exp, "%s %s cutoff %r" % (measure, side, c))


def test_cdist_gpu_every_string_slow(ctx):
    Q, Cs = ["é" * 3, "y" * 33], ["è", "z" * 34, "é" * 3]
    for measure in MEASURES:
        _assert_same(_run(ctx, measure, Q, Cs), R.score_matrix(measure, Q, Cs), measure)
        _assert_same(_run(ctx, measure, Q, ["ab", "abc"]), R.score_matrix(measure, Q, ["ab", "abc"]), measure)
        _assert_same(_run(ctx, measure, ["ab", "abc"], Cs), R.score_matrix(measure, ["ab", "abc"], Cs), measure)


# ---- the cutoff ---------------------------------------------------------------------------------------------------------------

def test_cdist_gpu_cutoff_at_an_attained_score_and_its_neighbours(ctx):
    # "ab" / "ba" is 0.5 under indel: kept at a cutoff of 0.5 and of the double below it, zeroed at the double above
    Q, Cs = ["ab", "abc", ""], ["ba", "ab", "", "abd"]
    M = R.score_matrix("ratio", Q, Cs)
    assert M[0, 0] == 0.5
    for cut, kept in ((math.nextafter(0.5, -INF), 0.5), (0.5, 0.5), (math.nextafter(0.5, INF), 0.0)):
        got = _run(ctx, "ratio", Q, Cs, cut)
        assert got[0, 0] == kept
        _assert_same(got, R.apply_cutoff(M, cut), "cutoff %r" % cut)


@pytest.mark.parametrize("measure", MEASURES)
def test_cdist_gpu_cutoffs(ctx, measure):
    Q, Cs, M = _edge_frame(measure)
    Q, Cs, M = Q[:130], Cs[:35], M[:130, :35]
    for cut in (-INF, 0.0, 0.3, 0.5, 0.8, 1.0, 1.5):
        got = _run(ctx, measure, Q, Cs, cut)
        _assert_same(got, R.apply_cutoff(M, cut), "%s cutoff %r" % (measure, cut))
        if cut == 1.5:
            assert not got.any()
        if cut in (-INF, 0.0):
            _assert_same(got, M, measure)
        if cut == 1.0:
            assert set(np.unique(got)) <= {0.0, 1.0}


# ---- token_sort_ratio ---------------------------------------------------------------------------------------------------------

def test_cdist_gpu_token_sort_ratio_over_token_frames(ctx):
    A, B = token_ref.gen_frame(141, 90)
    Q, Cs = A + ["  york\tnew\nmets ", "", "   "], B[:50] + ["mets new york", "", "z" * 20 + "          " + "y" * 12]
    M = R.score_matrix("token_sort_ratio", Q, Cs)
    _assert_same(_run(ctx, "token_sort_ratio", Q, Cs), M, "token_sort_ratio")
    _assert_same(_run(ctx, "token_sort_ratio", Q, Cs, 0.6), R.apply_cutoff(M, 0.6), "token_sort_ratio 0.6")
    # the same matrix over the columns normalised by the GPU's own transform
    _assert_same(_run(ctx, "ratio", S.token_sort(Q, ctx=ctx), S.token_sort(Cs, ctx=ctx)), M, "ratio of token_sort")


# ---- relations between GPU results --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _relation_frame(measure):
    Q = _frame(measure, 151, 150) + ["héllo wörld", "q" * 40, "a  b"]
    Cs = _frame(measure, 152, 90) + ["wörld hello", "q" * 39, "b a"]
    return Q, Cs


@pytest.mark.parametrize("measure", MEASURES)
def test_cdist_gpu_equals_the_exploded_pairwise_call(ctx, measure):
    Q, Cs = _relation_frame(measure)
    got = _run(ctx, measure, Q, Cs)
    qo, qv = S.pack_strings([q for q in Q for _ in Cs])
    co, cv = S.pack_strings(list(Cs) * len(Q))
    v = ctx.pairs_host(R.MEASURE[measure], qo, qv, co, cv)
    _assert_same(got, v.reshape(len(Q), len(Cs)), measure)


@pytest.mark.parametrize("measure", MEASURES)
def test_cdist_gpu_row_top4_equals_the_search(ctx, measure):
    Q, Cs = _relation_frame(measure)
    qo, qv = S.pack_strings(Q)
    co, cv = S.pack_strings(Cs)
    for cut in (None, 0.5):
        got = _run(ctx, measure, Q, Cs)
        if measure in ("ratio", "token_sort_ratio"):
            idx, score = ctx.extract(R.MEASURE[measure], qo, qv, co, cv, 4, cut)
        else:
            idx, score = ctx.best_match(measure, qo, qv, co, cv, 4, cut)
        ei, es = best_match_ref.topk(got, 4, cut)
        assert np.array_equal(np.where(idx == 0xFFFFFFFF, -1, idx.astype(np.int64)), ei)
        assert np.array_equal(score.view(np.uint64), es.view(np.uint64))


@pytest.mark.parametrize("measure", MEASURES)
def test_cdist_gpu_transpose_and_back_to_back_calls(ctx, measure):
    Q, Cs = _relation_frame(measure)
    a = _run(ctx, measure, Q, Cs, 0.3)
    b = _run(ctx, measure, Cs, Q, 0.3)
    _assert_same(a, b.T, measure)
    _assert_same(_run(ctx, measure, Q, Cs, 0.3), a, measure)
    # two device calls back to back on one context, read after one synchronize
    torch = pytest.importorskip("torch")
    cols = _device_columns(torch, *S.pack_strings(Q), *S.pack_strings(Cs))
    x = ctx.cdist(R.MEASURE[measure], *cols, score_cutoff=0.3)
    y = ctx.cdist(R.MEASURE[measure], cols[2], cols[3], cols[0], cols[1], score_cutoff=0.3)
    ctx.synchronize()
    _assert_same(x.cpu().numpy(), a, measure)
    _assert_same(y.cpu().numpy(), b, measure)


def test_cdist_gpu_enqueues_the_same_operations_whatever_the_size(ctx):
    # without slow strings a call is the packing, the read-back of the slow counts and one sweep, at any size
    torch = pytest.importorskip("torch")
    ops = {}
    for measure in ("levenshtein", "ratio"):
        for q, c in ((10, 10), (300, 700)):
            Q, Cs = _strings(161, q), _strings(162, c)
            cols = _device_columns(torch, *S.pack_strings(Q), *S.pack_strings(Cs))
            ctx.cdist(R.MEASURE[measure], *cols)  # (the first call of a measure may upload its table)
            ctx.synchronize()
            before = ctx.enqueued_ops
            out = ctx.cdist(R.MEASURE[measure], *cols)
            ops[measure, q] = ctx.enqueued_ops - before
            ctx.synchronize()
            assert out.shape == (q, c)
        assert ops[measure, 10] == ops[measure, 300] == 5


def test_cdist_gpu_python_wrapper_nulls_and_processor(ctx):
    Q = ["kitten", None, "abc"]
    Cs = [None, "sitting", "abd", None, "kitten"]
    M = S.cdist("ratio", Q, Cs, ctx=ctx)
    assert M.shape == (3, 5) and np.isnan(M[1]).all() and np.isnan(M[:, 0]).all() and np.isnan(M[:, 3]).all()
    assert M[0, 4] == 1.0 and M[0, 1] == E(5, 13) and M[2, 2] == E(2, 6)
    assert R.same(S.cdist("indel", Q, Cs, ctx=ctx), M)
    Z = S.cdist("ratio", Q, Cs, score_cutoff=0.7, ctx=ctx)
    assert Z[0, 4] == 1.0 and Z[0, 1] == 0.0 and Z[2, 2] == 0.0 and np.isnan(Z[1]).all()
    P = S.cdist("ratio", ["Apple, Inc."], ["apple  inc", "APPLE__INC"], ctx=ctx, processor="default_process")
    assert P[0, 0] == 1.0 and P[0, 1] < 1.0
    assert S.cdist("jaro", [], ["a"], ctx=ctx).shape == (0, 1) and S.cdist("jaro", ["a"], [None], ctx=ctx).shape == (1, 1)
