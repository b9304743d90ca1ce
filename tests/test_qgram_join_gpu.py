"""qgram_join on the MI355X (strsim_qgram_join_*) against the contract stated independently (tests/qgram_join_ref.py): qgram_ref's
score of every pair, then a brute-force CSR.  Everything is compared exactly: indptr, the candidate indices in ascending order, and
the scores bit for bit.  The frames (tests/qgram_join_frames.py) are the smallest at which each mechanism can go wrong, and every
parity frame is first shown not to be vacuous on the reference side: 0 < nnz < nq * nc."""
import ctypes as C

import numpy as np
import pytest

import qgram_join_frames as F
import qgram_join_ref as R

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")
KINDS = R.KINDS
GUARD_I = 0x5EA1F00D
GUARD_S = 0x7FF8C0FFEE15BAD1  # a NaN payload no score has


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def _run(ctx, kind, Q, Cs, cut=None, upper=False, q=2, multiset=True, **kw):
    got = ctx.qgram_join(kind, *S.pack_strings(Q), *S.pack_strings(Cs), cut, upper, q=q, multiset=multiset, **kw)
    assert got[0].shape == (len(Q) + 1,) and got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float64
    return got


def _assert_same(got, exp, what=""):
    gp, gi, gs = got
    ep, ei, es = exp
    assert np.array_equal(gp.astype(np.uint64), ep), "%s: indptr differs, first row %d" % (what, int(np.flatnonzero(gp.astype(np.uint64) != ep)[0]))
    assert np.array_equal(gi, ei), "%s: indices differ" % what
    assert np.array_equal(np.ascontiguousarray(gs).view(np.uint64), es.view(np.uint64)), "%s: scores differ" % what


def _device_columns(torch, *cols):
    dev = torch.device("cuda", 0)
    out = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.uint8)).to(dev) for x in cols]
    torch.cuda.synchronize()
    return out


# ---- 1. known answers: every kind x mode x q ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("q,multiset", F.MODES)
def test_qgram_join_gpu_known_answers(ctx, kind, q, multiset):
    X = F.KNOWN_STRINGS
    M = F.known_matrix(kind, q, multiset)
    assert F.not_vacuous(M, F.KNOWN_CUT)
    _assert_same(_run(ctx, kind, X, X, F.KNOWN_CUT, q=q, multiset=multiset), R.from_scores(M, F.KNOWN_CUT), "%s q=%d %r" % (kind, q, multiset))
    for a, b, k, kq, ms, want in R.KNOWN:
        if (k, kq, ms) != (kind, q, multiset):
            continue
        assert _run(ctx, kind, [a], [b], want, q=q, multiset=multiset)[2].tolist() == [want]      # in at its own score
        assert _run(ctx, kind, [a], [b], np.nextafter(want, 2.0), q=q, multiset=multiset)[0].tolist() == [0, 0]  # out at the next double


def test_qgram_join_gpu_anagrams_leave_at_any_positive_cutoff(ctx):
    # what match_join's jaccard cannot do: "abc" and "cba" share no bigram
    assert _run(ctx, "sorensen_dice", ["abc"], ["cba"], 5e-324)[0].tolist() == [0, 0]
    assert _run(ctx, "sorensen_dice", ["abc"], ["cba"], 0.0)[0].tolist() == [0, 1]
    assert _run(ctx, "sorensen_dice", ["abc"], ["cba"], 1.0, q=1)[2].tolist() == [1.0]


# ---- 2. the boundary frame -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("q,multiset", F.MODES)
def test_qgram_join_gpu_boundary_frame(ctx, kind, q, multiset):
    # lengths 0, q - 1, q, q + 1, 31, 32, 33; equal strings shorter than q; NULs; repeated grams; both plane forms; the fallback
    Q, Cs = F.boundary(q)
    M = F.boundary_matrix(kind, q, multiset)
    for cut in (F.BOUNDARY_CUT, 1.0):
        assert F.not_vacuous(M, cut)
        _assert_same(_run(ctx, kind, Q, Cs, cut, q=q, multiset=multiset), R.from_scores(M, cut), "%s q=%d %r at %r" % (kind, q, multiset, cut))
    assert F.not_vacuous(M, F.BOUNDARY_CUT, True)
    _assert_same(_run(ctx, kind, Q, Cs, F.BOUNDARY_CUT, True, q=q, multiset=multiset), R.from_scores(M, F.BOUNDARY_CUT, True), "upper")


# ---- 3. geometry: wave, workgroup and split edges --------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", F.GEOMETRY_NQ)
@pytest.mark.parametrize("nc", F.GEOMETRY_NC)
@pytest.mark.parametrize("upper", [False, True])
def test_qgram_join_gpu_geometry(ctx, nq, nc, upper):
    for kind, q, multiset in (("sorensen_dice", 2, True), ("jaccard", 3, False)):
        Q, Cs, M = F.geometry(kind, q, multiset, nq, nc)
        assert F.not_vacuous(M, F.GEOMETRY_CUT, upper)
        got = _run(ctx, kind, Q, Cs, F.GEOMETRY_CUT, upper, q=q, multiset=multiset)
        _assert_same(got, R.from_scores(M, F.GEOMETRY_CUT, upper), "%s %d x %d upper=%r" % (kind, nq, nc, upper))
        if upper:
            rows = np.repeat(np.arange(nq), np.diff(got[0]).astype(np.int64))
            assert (rows < got[1]).all()


# ---- 4. cutoffs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_qgram_join_gpu_cutoffs(ctx, kind):
    Q, Cs, M = F.geometry(kind, 2, True, 65, 300)
    n = []
    for cut in (None, -np.inf, 0.0, 0.6, 1.0, 1.5):
        got = _run(ctx, kind, Q, Cs, cut)
        _assert_same(got, R.from_scores(M, cut), "%s at %r" % (kind, cut))
        n.append(int(got[0][-1]))
    assert F.not_vacuous(M, 0.6) and F.not_vacuous(M, 1.0)
    assert n[0] == n[1] == n[2] == 65 * 300 and n[5] == 0 and 0 < n[4] < n[3] < n[2]


def test_qgram_join_gpu_a_cutoff_above_one_enqueues_one_operation(ctx):
    torch = pytest.importorskip("torch")
    L = S.lib()
    X = F.near_duplicates()
    cols = _device_columns(torch, *S.pack_strings(X[:100]), *S.pack_strings(X[:90]))
    for kind in KINDS:
        for q, multiset in F.MODES:
            ctx.synchronize()
            n0 = L.strsim_ctx_enqueued_ops(ctx._h)
            indptr, index, score = ctx.qgram_join(kind, *cols, 1.5, q=q, multiset=multiset)
            assert L.strsim_ctx_enqueued_ops(ctx._h) - n0 == 1
            ctx.synchronize()
            assert indptr.is_cuda and not indptr.cpu().numpy().any() and index.numel() == 0


def test_qgram_join_gpu_launch_counts(ctx):
    # multiset mode enqueues what match_join enqueues (16 for the count-only call, 18 with the fill and one sort launch); set mode
    # one kernel more in the count: the candidates' first occurrences
    torch = pytest.importorskip("torch")
    L = S.lib()
    X = F.near_duplicates()
    cols = _device_columns(torch, *S.pack_strings(X[:100]), *S.pack_strings(X[:90]))
    ops = lambda: L.strsim_ctx_enqueued_ops(ctx._h)
    for multiset, extra in ((True, 0), (False, 1)):
        ctx.synchronize()
        n0 = ops()
        ctx.qgram_join("sorensen_dice", *cols, 0.6, multiset=multiset, count_only=True)
        n1 = ops()
        ctx.qgram_join("sorensen_dice", *cols, 0.6, multiset=multiset, capacity=100 * 90)
        n2 = ops()
        ctx.synchronize()
        assert (n1 - n0, n2 - n1) == (16 + extra, 18 + extra)
    n0 = ops()
    ctx.match_join("sorensen_dice", *cols, 0.6, count_only=True)  # the existing family's count is what it was
    assert ops() - n0 == 16


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------------

def _raw_device_call(ctx, torch, kind_id, q, qflags, cols, nq, nc, cut, flags, capacity, room):
    """strsim_qgram_join_device with guard values in every output; -> (rc, nnz, indptr, index raw, score raw as uint64)"""
    dev = cols[0].device
    indptr = torch.full((nq + 1,), -7, dtype=torch.int64, device=dev)
    index = torch.from_numpy(np.full(room, GUARD_I, dtype=np.uint32).view(np.int32)).to(dev)
    score = torch.from_numpy(np.full(room, GUARD_S, dtype=np.uint64).view(np.int64)).to(dev)
    nnz = C.c_uint64(123456789)
    rc = S.lib().strsim_qgram_join_device(ctx._h, kind_id, q, qflags, cols[0].data_ptr(), cols[1].data_ptr(), nq, cols[2].data_ptr(),
                                          cols[3].data_ptr(), nc, cut, flags, capacity, indptr.data_ptr(), index.data_ptr() if capacity else None,
                                          score.data_ptr() if capacity else None, C.byref(nnz))
    ctx.synchronize()
    return rc, nnz.value, indptr.cpu().numpy().astype(np.uint64), index.cpu().numpy().view(np.uint32), score.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("multiset", [True, False])
@pytest.mark.parametrize("slow", [False, True])
def test_qgram_join_gpu_capacity_protocol(ctx, multiset, slow):
    torch = pytest.importorskip("torch")
    Q, Cs, M = F.geometry("sorensen_dice", 2, multiset, 130, 100) if multiset else F.geometry("jaccard", 3, multiset, 130, 100)
    kind, q = ("sorensen_dice", 2) if multiset else ("jaccard", 3)
    if slow:
        Q, Cs = list(Q), list(Cs)
        Q[5], Cs[9] = Q[5] + "q" * 40, "çà et là"
        M = R.score_matrix(kind, Q, Cs, q, multiset)
    ep, ei, es = R.from_scores(M, 0.6)
    n = int(ep[-1])
    assert 100 < n < 130 * 100
    kid, flags = KINDS.index(kind), 0 if multiset else 1
    cols = _device_columns(torch, *S.pack_strings(Q), *S.pack_strings(Cs))
    # exact, guard elements behind both outputs
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, kid, q, flags, cols, len(Q), len(Cs), 0.6, 0, n, n + 16)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and np.array_equal(index[:n], ei) and np.array_equal(score[:n], es.view(np.uint64))
    assert (index[n:] == GUARD_I).all() and (score[n:] == GUARD_S).all()
    # one less: indptr and nnz are still exact, not one element of the outputs is touched
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, kid, q, flags, cols, len(Q), len(Cs), 0.6, 0, n - 1, n + 16)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and (index == GUARD_I).all() and (score == GUARD_S).all()
    # count only: zero with NULL outputs
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, kid, q, flags, cols, len(Q), len(Cs), 0.6, 0, 0, 8)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and (index == GUARD_I).all() and (score == GUARD_S).all()
    # the binding's retry: a guess that is too small, then the exact size; and its count-only form
    _assert_same(_run(ctx, kind, Q, Cs, 0.6, q=q, multiset=multiset, capacity=3), (ep, ei, es), "retry")
    assert np.array_equal(ctx.qgram_join(kind, *S.pack_strings(Q), *S.pack_strings(Cs), 0.6, q=q, multiset=multiset, count_only=True), ep)


# ---- 6. relations to untouched kernels -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["jaccard", "sorensen_dice"])
def test_qgram_join_gpu_unigram_multiset_equals_match_join(ctx, kind):
    # at q = 1 in multiset mode the scores are measures 3 and 4, bit for bit: the whole CSR equals match_join's, on 300 x 300
    X = list(F.near_duplicates())
    cols = (*S.pack_strings(X), *S.pack_strings(X))
    for cut, upper in ((0.8, False), (0.9, True), (1.0, False)):
        want = ctx.match_join(kind, *cols, cut, upper)
        assert 0 < want[1].size < 300 * 300
        _assert_same(ctx.qgram_join(kind, *cols, cut, upper, q=1, multiset=True), tuple(np.asarray(x) for x in want), "%s at %r" % (kind, cut))


@pytest.mark.parametrize("kind,q,multiset", [("sorensen_dice", 2, True), ("cosine", 3, True), ("overlap", 2, False), ("jaccard", 1, False)])
def test_qgram_join_gpu_equals_the_pairwise_call(ctx, kind, q, multiset):
    # every pair through strsim_qgram_host as explicit pair columns: every reported score is the pairwise call's, and every pair the
    # pairwise call scores at or above the cutoff is reported
    Q, Cs = F.boundary(q)
    Q, Cs = list(Q) + list(F.near_duplicates()[:40]), list(Cs) + list(F.near_duplicates()[20:80])
    A = [s for s in Q for _ in Cs]
    B = Cs * len(Q)
    P = ctx.qgram_host(kind, *S.pack_strings(A), *S.pack_strings(B), q, multiset).reshape(len(Q), len(Cs))
    for cut in (0.3, 0.8):
        exp = R.from_scores(P, cut)
        assert 0 < exp[1].size < P.size
        _assert_same(_run(ctx, kind, Q, Cs, cut, q=q, multiset=multiset), exp, "%s q=%d at %r" % (kind, q, cut))


@pytest.mark.parametrize("kind,q,multiset", [("overlap", 1, True), ("overlap", 2, True), ("overlap", 3, True), ("jaccard", 2, False),
                                             ("sorensen_dice", 3, False), ("cosine", 1, False), ("overlap", 2, False)])
def test_qgram_join_gpu_unpruned_masks_are_still_right(ctx, kind, q, multiset):
    # overlap and set mode visit every length with a gram: the results at a cutoff equal brute force
    Q, Cs, M = F.geometry(kind, q, multiset, 65, 300)
    for cut in (0.8, 1.0):
        assert F.not_vacuous(M, cut)
        _assert_same(_run(ctx, kind, Q, Cs, cut, q=q, multiset=multiset), R.from_scores(M, cut), "%s q=%d %r at %r" % (kind, q, multiset, cut))


# ---- 7. entry points -------------------------------------------------------------------------------------------------------------

def test_qgram_join_gpu_device_and_host_entry_points_between_other_calls(ctx):
    torch = pytest.importorskip("torch")
    Q, Cs, M = F.geometry("sorensen_dice", 2, True, 100, 90)
    exp = R.from_scores(M, 0.8)
    assert F.not_vacuous(M, 0.8)
    host = (*S.pack_strings(Q), *S.pack_strings(Cs))
    dev = _device_columns(torch, *host)
    before = ctx.pairs_host("levenshtein", *S.pack_strings(Q[:50]), *S.pack_strings(Cs[:50]))
    pair = ctx.qgram_host("sorensen_dice", *S.pack_strings(Q[:50]), *S.pack_strings(Cs[:50]))
    _assert_same(ctx.qgram_join("sorensen_dice", *host, 0.8), exp, "host")
    mj = ctx.match_join("jaro", *host, 0.9)
    indptr, index, score = ctx.qgram_join("sorensen_dice", *dev, 0.8)
    ctx.synchronize()
    assert indptr.is_cuda and index.is_cuda and score.is_cuda
    _assert_same((indptr.cpu().numpy().astype(np.uint64), index.cpu().numpy().view(np.uint32), score.cpu().numpy()), exp, "device")
    setm = ctx.qgram_join("jaccard", *dev, 0.8, q=3, multiset=False)  # set mode, then multiset again: the buffers are the context's
    ctx.synchronize()
    _assert_same((setm[0].cpu().numpy().astype(np.uint64), setm[1].cpu().numpy().view(np.uint32), setm[2].cpu().numpy()),
                 R.from_scores(np.ascontiguousarray(F.near_matrix("jaccard", 3, False)[:100, :90]), 0.8), "set mode")
    _assert_same(ctx.qgram_join("sorensen_dice", *host, 0.8), exp, "host again")
    # the calls around it give what they gave
    assert np.array_equal(ctx.pairs_host("levenshtein", *S.pack_strings(Q[:50]), *S.pack_strings(Cs[:50])).view(np.uint64), before.view(np.uint64))
    assert np.array_equal(ctx.qgram_host("sorensen_dice", *S.pack_strings(Q[:50]), *S.pack_strings(Cs[:50])).view(np.uint64), pair.view(np.uint64))
    again = ctx.match_join("jaro", *host, 0.9)
    assert all(np.array_equal(a, b) for a, b in zip(mj, again)) and mj[1].size > 0


def test_qgram_join_gpu_edge_shapes(ctx):
    for Q, Cs in (([], ["a"]), (["a"], []), ([], [])):
        indptr, index, score = _run(ctx, "jaccard", Q, Cs, 0.5)
        assert indptr.tolist() == [0] * (len(Q) + 1) and index.size == 0 and score.size == 0
    _assert_same(_run(ctx, "cosine", ["", "a"], ["", "a", "b"], 0.5), R.join("cosine", ["", "a"], ["", "a", "b"], 0.5), "empty strings")
    _assert_same(_run(ctx, "overlap", ["", ""], ["", "", ""], 1.0, q=3, multiset=False), R.join("overlap", ["", ""], ["", "", ""], 1.0, 3, False),
                 "only empty strings")


# ---- 8. the Python surface -------------------------------------------------------------------------------------------------------

def test_qgram_join_gpu_python_surface_nulls_and_dedupe(ctx):
    Q = ["night", None, "abc", "nigh"]
    Cs = [None, "night", "abc", None, "nacht", "nights"]
    indptr, index, score = S.qgram_join("sorensen_dice", Q, Cs, 0.5, ctx=ctx)
    assert indptr.dtype == np.int64 and index.dtype == np.int64 and score.dtype == np.float64
    assert indptr.tolist() == [0, 2, 2, 3, 5] and index.tolist() == [1, 5, 2, 1, 5]
    assert score.tolist() == [1.0, 8.0 / 9.0, 1.0, 6.0 / 7.0, 0.75]
    X = list(F.near_duplicates()[:80])
    M = np.ascontiguousarray(F.near_matrix("sorensen_dice", 2, True)[:80, :80])
    ep, ei, es = R.from_scores(M, 0.8, True)
    assert 0 < ei.size
    i, j, s = S.qgram_dedupe_pairs("sorensen_dice", X, 0.8, ctx=ctx)
    assert np.array_equal(i, np.repeat(np.arange(80), np.diff(ep.astype(np.int64)))) and np.array_equal(j, ei.astype(np.int64))
    assert np.array_equal(s.view(np.uint64), es.view(np.uint64))
    with pytest.raises(ValueError, match="unknown q-gram kind"):
        S.qgram_join("ratio", Q, Cs, 0.5, ctx=ctx)


def test_qgram_join_gpu_fallback_leaves_last_wave_rows_alone(ctx):
    # the fallback's internal pairwise calls do not change what strsim_ctx_last_wave_rows reports of the caller's own last call
    A, B = ["müller", "abc", "x" * 70], ["muller", "abd", "x" * 69]
    ctx.qgram_host("jaccard", *S.pack_strings(A), *S.pack_strings(B))
    assert ctx.last_wave_rows == 2
    Q, Cs = ["night", "müller", "a" * 40], ["nacht", "night", "muller", "a" * 41, "日本"]
    _assert_same(_run(ctx, "sorensen_dice", Q, Cs, 0.2), R.join("sorensen_dice", Q, Cs, 0.2), "slow on both sides")
    assert ctx.last_wave_rows == 2
