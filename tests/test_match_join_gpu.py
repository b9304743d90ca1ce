"""match_join on the MI355X (strsim_match_join_*) against the contract stated independently (tests/match_join_ref.py): the CPU
oracle's score of every pair, then a brute-force CSR.  Everything is compared exactly: indptr, the candidate indices in ascending
order, and the scores bit for bit.  The shapes are the smallest at which each mechanism can go wrong: several splits with a last wave
of one live lane, several candidates per (length, split) slice, every length 0 .. 32 on both sides, both plane counts, every mix of
strings inside and outside the lane class, the long sort tier."""
import ctypes as C
import functools
import math
import random

import numpy as np
import pytest

import match_join_ref as R
import process_ref

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")
MEASURES = R.MEASURES
GUARD_I = 0x5EA1F00D
GUARD_S = 0x7FF8C0FFEE15BAD1  # a NaN payload no score has
LOWER = "abcdefghijklmnopqrstuvwxyz"
MIXED = LOWER + LOWER.upper() + "0123456789" + " .,-_'/&()"


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def _run(ctx, measure, Q, Cs, cut=None, upper=False, **kw):
    got = ctx.match_join(measure, *S.pack_strings(Q), *S.pack_strings(Cs), cut, upper, **kw)
    assert got[0].shape == (len(Q) + 1,) and got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float64
    return got


def _assert_same(got, exp, what=""):
    gp, gi, gs = got
    ep, ei, es = exp
    assert np.array_equal(gp.astype(np.uint64), ep), "%s: indptr differs, first row %d" % (what, int(np.flatnonzero(gp.astype(np.uint64) != ep)[0]))
    assert np.array_equal(gi, ei), "%s: indices differ" % what
    assert np.array_equal(np.ascontiguousarray(gs).view(np.uint64), es.view(np.uint64)), "%s: scores differ" % what


def _candidates(rng, n, alphabet):
    """n strings whose lengths cycle through 0 .. 32 (every length present from n = 33 on), a shared stem of 0 .. 5 characters first"""
    stem = "".join(rng.choice(alphabet) for _ in range(5))
    out = []
    for k in range(n):
        ln = k % 33
        pre = stem[:min(rng.randint(0, 5), ln)]
        out.append(pre + "".join(rng.choice(alphabet) for _ in range(ln - len(pre))))
    return out


def _edited(rng, s, alphabet, edits):
    s = list(s)
    for _ in range(edits):
        op = rng.randrange(4)
        p = rng.randrange(len(s) + 1)
        if op == 0 and len(s) < 32:
            s.insert(p, rng.choice(alphabet))
        elif op == 1 and s:
            del s[min(p, len(s) - 1)]
        elif op == 2 and s:
            s[min(p, len(s) - 1)] = rng.choice(alphabet)
        elif op == 3 and len(s) >= 2:  # an adjacent swap: a Jaro transposition
            p = min(p, len(s) - 2)
            s[p], s[p + 1] = s[p + 1], s[p]
    return "".join(s)


def _queries(rng, Cs, n, alphabet):
    """every length 0 .. 32 first (a candidate of that length with one adjacent swap), then candidates with 0 .. 3 edits"""
    by_len = {len(c): c for c in Cs}
    out = [_edited(rng, by_len[ln], alphabet, 0) if ln < 2 else "".join(by_len[ln][1::-1]) + by_len[ln][2:] for ln in range(33)]
    while len(out) < n:
        out.append(_edited(rng, rng.choice(Cs), alphabet, rng.randint(0, 3)))
    return out[:n]


@functools.lru_cache(maxsize=None)
def _frame(name):
    """(Q, Cs) of a named frame; generated once"""
    nq, nc, alphabet, seed = {"257x129": (257, 129, LOWER, 11), "130x600": (130, 600, LOWER, 12), "mixed": (70, 99, MIXED, 13)}[name]
    rng = random.Random(seed)
    Cs = _candidates(rng, nc, alphabet)
    Q = _queries(rng, Cs, nq, alphabet)
    assert {len(s) for s in Q} >= set(range(33)) and {len(s) for s in Cs} >= set(range(33))
    return Q, Cs


@functools.lru_cache(maxsize=None)
def _scores(name, measure):
    """the oracle's matrix of a frame: computed once, shared, read-only"""
    Q, Cs = _frame(name)
    M = R.score_matrix(measure, Q, Cs)
    M.setflags(write=False)
    return M


def _cuts(M):
    """none, 0, 0.5, 0.8, 1.0, 1.5, and the exact score of one known pair with both its f64 neighbours"""
    inner = M[(M > 0.5) & (M < 1.0)]
    assert inner.size
    e = float(inner[inner.size // 2])
    return (None, 0.0, 0.5, 0.8, 1.0, 1.5, math.nextafter(e, 0.0), e, math.nextafter(e, 2.0))


def _device_columns(torch, *cols):
    dev = torch.device("cuda", 0)
    out = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.uint8)).to(dev) for x in cols]
    torch.cuda.synchronize()
    return out


# ---- 1. the base frames -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("name", ["257x129", "130x600"])
def test_match_join_gpu_base_frame(ctx, measure, name):
    # 257 x 129: three splits on 256 CUs and a last wave of one live lane; 130 x 600: several candidates per (length, split) slice
    Q, Cs = _frame(name)
    M = _scores(name, measure)
    n = []
    for cut in _cuts(M):
        got = _run(ctx, measure, Q, Cs, cut)
        _assert_same(got, R.from_scores(M, cut), "%s %s at %r" % (measure, name, cut))
        n.append(int(got[0][-1]))
    assert n[0] == n[1] == len(Q) * len(Cs) and n[5] == 0
    assert n[6] == n[7] > n[8]  # the known pair is a hit at its own score and leaves at the next double
    assert 0 < n[3] < n[2] < n[1]


@pytest.mark.parametrize("measure", MEASURES)
def test_match_join_gpu_base_frame_upper(ctx, measure):
    Q, Cs = _frame("257x129")
    M = _scores("257x129", measure)
    for cut in (None, 0.8):
        _assert_same(_run(ctx, measure, Q, Cs, cut, True), R.from_scores(M, cut, True), "%s upper at %r" % (measure, cut))


# ---- 2. the plane choice ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", MEASURES)
def test_match_join_gpu_seven_planes(ctx, measure):
    # case, digits and punctuation: bits 5 and 6 disagree inside a pair
    Q, Cs = _frame("mixed")
    M = _scores("mixed", measure)
    for cut in (None, 0.5, 0.8):
        _assert_same(_run(ctx, measure, Q, Cs, cut), R.from_scores(M, cut), "%s mixed at %r" % (measure, cut))


@pytest.mark.parametrize("measure", MEASURES)
def test_match_join_gpu_one_upper_case_candidate_among_lower_case(ctx, measure):
    # the wave's queries are five-plane material, one candidate is not: the choice is made per candidate
    Q, Cs = _frame("257x129")
    Q, Cs = list(Q[:70]), list(Cs[:66])
    Cs[40] = Q[12].upper()
    Cs[41] = Q[12]
    M = R.score_matrix(measure, Q, Cs)
    for cut in (0.0, 0.7, 1.0):
        got = _run(ctx, measure, Q, Cs, cut)
        _assert_same(got, R.from_scores(M, cut), "%s at %r" % (measure, cut))
    assert 41 in got[1][int(got[0][12]):int(got[0][13])].tolist() and 40 not in got[1][int(got[0][12]):int(got[0][13])].tolist()


# ---- 3. strings outside the lane class ----------------------------------------------------------------------------------------

LONG33 = "abcdefghij klmnopqrst uvwxyzabcde"
SLOW = [LONG33, "x" * 40, "müller", "mueller and sons, a firm well beyond the lane"]


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("side", ["query", "candidate", "both", "all", "none"])
def test_match_join_gpu_slow_strings(ctx, measure, side):
    # 33 and 40 ASCII bytes and non-ASCII go through the pairwise call; near copies of them are hits across the classes
    assert len(LONG33.encode()) == 33
    Q, Cs = _frame("257x129")
    Q, Cs = list(Q[:70]), list(Cs[:45])
    Q[5], Cs[7] = "muller", LONG33[:32]
    if side in ("query", "both"):
        Q[33], Q[64], Q[69] = LONG33, "müller", "x" * 40
    if side in ("candidate", "both"):
        Cs[17], Cs[0], Cs[44] = "müller", "x" * 39 + "y", LONG33
    if side == "all":
        Q = [s + " %02d" % k for k, s in enumerate(SLOW * 3)]
        Cs = [s + " %02d" % k for k, s in enumerate(SLOW[::-1] * 2)]
    M = R.score_matrix(measure, Q, Cs)
    for cut in (None, 0.5, 0.9):
        for upper in (False, True):
            _assert_same(_run(ctx, measure, Q, Cs, cut, upper), R.from_scores(M, cut, upper), "%s %s at %r" % (measure, side, cut))


# ---- 4. self-join -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", MEASURES)
def test_match_join_gpu_upper_self_join_and_dedupe(ctx, measure):
    Q, _ = _frame("257x129")
    base = list(Q[33:73])
    X = base + [_edited(random.Random(5), s, LOWER, 1) for s in base[:30]] + base[:20]  # identical strings at different positions
    M = R.score_matrix(measure, X, X)
    for cut in (0.0, 0.85, 1.0):
        indptr, index, score = got = _run(ctx, measure, X, X, cut, True)
        _assert_same(got, R.from_scores(M, cut, True), "%s upper at %r" % (measure, cut))
        rows = np.repeat(np.arange(len(X)), np.diff(indptr).astype(np.int64))
        assert (rows < index).all()  # each unordered pair once, never (i, i)
        i, j, s = S.match_dedupe_pairs(measure, X, cut, ctx=ctx)
        assert np.array_equal(i, rows) and np.array_equal(j, index.astype(np.int64)) and np.array_equal(s.view(np.uint64), score.view(np.uint64))
    assert {(k, 70 + k) for k in range(20)} <= set(zip(rows.tolist(), index.tolist()))


# ---- 5. capacity --------------------------------------------------------------------------------------------------------------

def _raw_device_call(ctx, torch, measure_id, cols, nq, nc, cut, flags, capacity, room):
    """strsim_match_join_device with guard values in every output; -> (rc, nnz, indptr, index raw, score raw as uint64)"""
    dev = cols[0].device
    indptr = torch.full((nq + 1,), -7, dtype=torch.int64, device=dev)
    index = torch.from_numpy(np.full(room, GUARD_I, dtype=np.uint32).view(np.int32)).to(dev)
    score = torch.from_numpy(np.full(room, GUARD_S, dtype=np.uint64).view(np.int64)).to(dev)
    nnz = C.c_uint64(123456789)
    rc = S.lib().strsim_match_join_device(ctx._h, measure_id, cols[0].data_ptr(), cols[1].data_ptr(), nq, cols[2].data_ptr(), cols[3].data_ptr(), nc,
                                          cut, flags, capacity, indptr.data_ptr(), index.data_ptr() if capacity else None,
                                          score.data_ptr() if capacity else None, C.byref(nnz))
    ctx.synchronize()
    return rc, nnz.value, indptr.cpu().numpy().astype(np.uint64), index.cpu().numpy().view(np.uint32), score.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("measure", ["levenshtein", "jaro_winkler"])
@pytest.mark.parametrize("slow", [False, True])
def test_match_join_gpu_capacity_protocol(ctx, measure, slow):
    torch = pytest.importorskip("torch")
    Q, Cs = _frame("257x129")
    Q, Cs = list(Q[:130]), list(Cs[:100])
    if slow:
        Q[5] = "q" * 40
        Cs[9] = "çà et là"
    mid = S.MEASURE_ID[measure]
    ep, ei, es = R.join(measure, Q, Cs, 0.5)
    n = int(ep[-1])
    assert n > 100
    cols = _device_columns(torch, *S.pack_strings(Q), *S.pack_strings(Cs))
    # exact, guard elements behind both outputs
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, mid, cols, len(Q), len(Cs), 0.5, 0, n, n + 16)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and np.array_equal(index[:n], ei) and np.array_equal(score[:n], es.view(np.uint64))
    assert (index[n:] == GUARD_I).all() and (score[n:] == GUARD_S).all()
    # one less: indptr and nnz are still exact, not one element of the outputs is touched
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, mid, cols, len(Q), len(Cs), 0.5, 0, n - 1, n + 16)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and (index == GUARD_I).all() and (score == GUARD_S).all()
    # count only: zero with NULL outputs
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, mid, cols, len(Q), len(Cs), 0.5, 0, 0, 8)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and (index == GUARD_I).all() and (score == GUARD_S).all()
    # the binding's retry: a guess that is too small, then the exact size; and its count-only form
    _assert_same(_run(ctx, measure, Q, Cs, 0.5, capacity=3), (ep, ei, es), "retry")
    assert np.array_equal(ctx.match_join(measure, *S.pack_strings(Q), *S.pack_strings(Cs), 0.5, count_only=True), ep)


# ---- 6. the sort's tiers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", MEASURES)
def test_match_join_gpu_long_sort_tier(ctx, measure):
    # rows of 700 hits: the long tier of the row sort behind the new sweep
    Q, Cs = _frame("130x600")
    Q = list(Q[40:43])
    Cs = list(Cs) + list(_frame("257x129")[1][:100])
    assert len(Cs) == 700
    indptr, index, score = got = _run(ctx, measure, Q, Cs, 0.0)
    _assert_same(got, R.join(measure, Q, Cs, 0.0), measure)
    assert indptr.tolist() == [0, 700, 1400, 2100] and np.array_equal(index, np.tile(np.arange(700, dtype=np.uint32), 3))


# ---- 7. edge shapes, launch counts and determinism ----------------------------------------------------------------------------

@pytest.mark.parametrize("measure", MEASURES)
def test_match_join_gpu_edge_shapes(ctx, measure):
    for Q, Cs in (([], ["a"]), (["a"], []), ([], [])):
        indptr, index, score = _run(ctx, measure, Q, Cs, 0.5)
        assert indptr.tolist() == [0] * (len(Q) + 1) and index.size == 0 and score.size == 0
    got = _run(ctx, measure, ["a"], ["a"], 1.0)
    assert got[0].tolist() == [0, 1] and got[1].tolist() == [0] and got[2].tolist() == [1.0]
    assert _run(ctx, measure, ["a"], ["b"], 0.5)[0].tolist() == [0, 0]
    _assert_same(_run(ctx, measure, ["", "a"], ["", "a", "b"], 0.5), R.join(measure, ["", "a"], ["", "a", "b"], 0.5), "empty strings")
    _assert_same(_run(ctx, measure, ["", ""], ["", "", ""], 1.0), R.join(measure, ["", ""], ["", "", ""], 1.0), "only empty strings")


def test_match_join_gpu_launch_counts_and_the_cutoff_above_one(ctx):
    # the operations of join, one for one: 16 for the count-only call, 18 with the fill and one sort launch; a cutoff above 1.0 is
    # one clear of indptr
    torch = pytest.importorskip("torch")
    L = S.lib()
    Q, Cs = _frame("257x129")
    cols = _device_columns(torch, *S.pack_strings(Q[:100]), *S.pack_strings(Cs[:90]))
    ops = lambda: L.strsim_ctx_enqueued_ops(ctx._h)
    for measure in MEASURES:
        ctx.synchronize()
        n0 = ops()
        ctx.match_join(measure, *cols, 0.6, count_only=True)
        n1 = ops()
        ctx.match_join(measure, *cols, 0.6, capacity=100 * 90)
        n2 = ops()
        indptr, index, score = ctx.match_join(measure, *cols, 1.5)
        n3 = ops()
        ctx.synchronize()
        assert (n1 - n0, n2 - n1, n3 - n2) == (16, 18, 1), measure
        assert indptr.is_cuda and not indptr.cpu().numpy().any() and index.numel() == 0


@pytest.mark.parametrize("measure", MEASURES)
def test_match_join_gpu_two_identical_calls_give_identical_bytes(ctx, measure):
    Q, Cs = _frame("130x600")
    a = _run(ctx, measure, Q, Cs, 0.7)
    b = _run(ctx, measure, Q, Cs, 0.7)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[1].size > 0


def test_match_join_gpu_device_columns_give_device_results(ctx):
    torch = pytest.importorskip("torch")
    Q, Cs = _frame("257x129")
    M = _scores("257x129", "jaro_winkler")
    cols = _device_columns(torch, *S.pack_strings(Q[:100]), *S.pack_strings(Cs[:90]))
    indptr, index, score = ctx.match_join("jaro_winkler", *cols, 0.9)
    ctx.synchronize()
    assert indptr.is_cuda and index.is_cuda and score.is_cuda
    _assert_same((indptr.cpu().numpy().astype(np.uint64), index.cpu().numpy().view(np.uint32), score.cpu().numpy()),
                 R.from_scores(np.ascontiguousarray(M[:100, :90]), 0.9), "device")


# ---- 8. the Python surface and the processor ----------------------------------------------------------------------------------

def test_match_join_gpu_python_surface_nulls(ctx):
    Q = ["anna", None, "bob", "anne"]
    Cs = [None, "anna", "bob", None, "anne", "bobby"]
    indptr, index, score = S.match_join("levenshtein", Q, Cs, 0.6, ctx=ctx)
    assert indptr.dtype == np.int64 and index.dtype == np.int64 and score.dtype == np.float64
    assert indptr.tolist() == [0, 2, 2, 4, 6] and index.tolist() == [1, 4, 2, 5, 1, 4]
    assert score.tolist() == [1.0, 0.75, 1.0, 0.6, 0.75, 1.0]
    with pytest.raises(ValueError, match="no match_join by measure"):
        S.match_join("ratio", Q, Cs, 0.5, ctx=ctx)


@pytest.mark.parametrize("measure", MEASURES)
def test_match_join_gpu_default_process(ctx, measure):
    Q = ["  Anna-Maria ", "BOB!", "anne", "O'Neil, J.", "müller", ""]
    Cs = ["anna maria", "bob", "Anne ", "o neil  j", "Müller", "MUELLER", "--"]
    PQ, PC = process_ref.default_process_column(Q), process_ref.default_process_column(Cs)
    for cut in (None, 0.8, 1.0):
        got = S.match_join(measure, Q, Cs, cut, ctx=ctx, processor="default_process")
        assert R.same(got, R.join(measure, PQ, PC, cut)), (measure, cut)
    i, j, s = S.match_dedupe_pairs(measure, Q + Cs, 1.0, ctx=ctx, processor="default_process")
    assert {(0, 6), (1, 7), (2, 8), (3, 9), (4, 10), (5, 12)} <= set(zip(i.tolist(), j.tolist()))
