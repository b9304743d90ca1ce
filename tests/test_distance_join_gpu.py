"""distance_join on the MI355X (strsim_distance_join_*) against the contract stated independently (tests/distance_join_ref.py): the
edit distance of every pair by plain DPs, then a brute-force CSR.  Everything is compared exactly: indptr, the candidate indices in
ascending order and the distances.  The frames (tests/distance_join_frames.py) are the smallest at which each mechanism can go
wrong, and every parity frame is first shown not to be vacuous on the reference side: 0 < nnz < the pairs."""
import ctypes as C

import numpy as np
import pytest

import distance_join_frames as F
import distance_join_ref as R

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")
MEASURES = R.MEASURES
GUARD_I = 0x5EA1F00D
GUARD_D = 0x7E57D157
UNBOUNDED = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def _run(ctx, measure, Q, Cs, k=None, upper=False, **kw):
    got = ctx.distance_join(measure, *S.pack_strings(Q), *S.pack_strings(Cs), k, upper, **kw)
    assert got[0].shape == (len(Q) + 1,) and got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.uint32
    return got


def _assert_same(got, exp, what=""):
    gp, gi, gd = got
    ep, ei, ed = exp
    assert np.array_equal(gp.astype(np.uint64), ep), "%s: indptr differs, first row %d" % (what, int(np.flatnonzero(gp.astype(np.uint64) != ep)[0]))
    assert np.array_equal(gi, ei), "%s: indices differ" % what
    assert np.array_equal(gd, ed), "%s: distances differ" % what


def _device_columns(torch, *cols):
    dev = torch.device("cuda", 0)
    out = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.uint8)).to(dev) for x in cols]
    torch.cuda.synchronize()
    return out


# ---- 1. known answers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", MEASURES)
def test_distance_join_gpu_known_answers(ctx, measure):
    X = F.KNOWN_STRINGS
    M = F.known_matrix(measure)
    for k in F.KS:
        assert F.not_vacuous(M, k)
        _assert_same(_run(ctx, measure, X, X, k), R.from_distances(M, k), "%s at %r" % (measure, k))
        _assert_same(_run(ctx, measure, X, X, k, True), R.from_distances(M, k, True), "%s at %r, upper" % (measure, k))
    for a, b, lev, osa, dl in R.KNOWN:
        d = (lev, osa, dl)[MEASURES.index(measure)]
        assert _run(ctx, measure, [a], [b], d)[2].tolist() == [d]              # in at its own distance
        if d:
            assert _run(ctx, measure, [a], [b], d - 1)[0].tolist() == [0, 0]   # out one below
        assert _run(ctx, measure, [a], [b], None)[2].tolist() == [d]


def test_distance_join_gpu_the_three_measures_part_at_ca_abc(ctx):
    # ("ca", "abc"): 3 / 3 / 2; ("ca", "ac"): 2 / 1 / 1
    got = [_run(ctx, m, ["ca"], ["abc", "ac"], 2) for m in MEASURES]
    assert [g[1].tolist() for g in got] == [[1], [1], [0, 1]] and [g[2].tolist() for g in got] == [[2], [1], [2, 1]]


# ---- 2. the boundary frame -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", MEASURES)
def test_distance_join_gpu_boundary_frame(ctx, measure):
    # lengths 0, 1, 31, 32, 33; | lq - lc | and d at k and k + 1; both plane forms; NULs; non-ASCII and 33-byte rows (the fallback);
    # a 32-byte candidate against 32-byte queries left undecided by the OSA distance
    Q, Cs = F.boundary()
    M = F.boundary_matrix(measure)
    for k in F.KS:
        assert F.not_vacuous(M, k)
        _assert_same(_run(ctx, measure, Q, Cs, k), R.from_distances(M, k), "%s at %r" % (measure, k))
    for k in (1, 2):
        assert F.not_vacuous(M, k, True)
        _assert_same(_run(ctx, measure, Q, Cs, k, True), R.from_distances(M, k, True), "%s at %r, upper" % (measure, k))
    # and the other way round: the slow strings and the 32-byte rows change sides
    for k in (0, 2, 3):
        _assert_same(_run(ctx, measure, Cs, Q, k), R.from_distances(np.ascontiguousarray(M.T), k), "%s transposed at %r" % (measure, k))


# ---- 3. geometry: wave, workgroup and split edges --------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", F.GEOMETRY_NQ)
@pytest.mark.parametrize("nc", F.GEOMETRY_NC)
@pytest.mark.parametrize("upper", [False, True])
def test_distance_join_gpu_geometry(ctx, nq, nc, upper):
    for measure in MEASURES:
        Q, Cs, M = F.geometry(measure, nq, nc)
        for k in F.geometry_ks(nq, nc):
            assert F.not_vacuous(M, k, upper)
            got = _run(ctx, measure, Q, Cs, k, upper)
            _assert_same(got, R.from_distances(M, k, upper), "%s %d x %d at %r upper=%r" % (measure, nq, nc, k, upper))
            if upper:
                rows = np.repeat(np.arange(nq), np.diff(got[0]).astype(np.int64))
                assert (rows < got[1]).all()


def test_distance_join_gpu_damerau_differs_from_osa_where_it_must(ctx):
    # the whole frame at k = 2 and 3: hits the OSA join does not have, at distances below the OSA distance
    X = list(F.near_duplicates())
    O, D = F.near_matrix("osa"), F.near_matrix("damerau_levenshtein")
    for k in (2, 3):
        below, misses, quiet = F.damerau_frame_report(tuple(X), k)
        assert below >= 20 and misses >= 20 and quiet >= 1
        got = _run(ctx, "damerau_levenshtein", X, X, k)
        _assert_same(got, R.from_distances(D, k), "damerau at %d" % k)
        osa = _run(ctx, "osa", X, X, k)
        assert int(got[0][-1]) - int(osa[0][-1]) == int(((D <= k) & (O > k)).sum()) > 0


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------------

def _raw_device_call(ctx, torch, kind_id, cols, nq, nc, k, flags, capacity, room):
    """strsim_distance_join_device with guard values in every output; -> (rc, nnz, indptr, index raw, distance raw)"""
    dev = cols[0].device
    indptr = torch.full((nq + 1,), -7, dtype=torch.int64, device=dev)
    index = torch.from_numpy(np.full(room, GUARD_I, dtype=np.uint32).view(np.int32)).to(dev)
    dist = torch.from_numpy(np.full(room, GUARD_D, dtype=np.uint32).view(np.int32)).to(dev)
    nnz = C.c_uint64(123456789)
    rc = S.lib().strsim_distance_join_device(ctx._h, kind_id, cols[0].data_ptr(), cols[1].data_ptr(), nq, cols[2].data_ptr(), cols[3].data_ptr(), nc,
                                             k, flags, capacity, indptr.data_ptr(), index.data_ptr() if capacity else None,
                                             dist.data_ptr() if capacity else None, C.byref(nnz))
    ctx.synchronize()
    return rc, nnz.value, indptr.cpu().numpy().astype(np.uint64), index.cpu().numpy().view(np.uint32), dist.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("slow", [False, True])
def test_distance_join_gpu_capacity_protocol(ctx, measure, slow):
    torch = pytest.importorskip("torch")
    Q, Cs, M = F.geometry(measure, 130, 100)
    if slow:
        Q, Cs = list(Q), list(Cs)
        Q[5], Cs[9] = Q[5] + "q" * 40, "çà et là"
        Q[6], Cs[10] = "ça et là", Cs[9 + 20] + "q" * 40
        M = R.matrix(measure, Q, Cs)
    ep, ei, ed = R.from_distances(M, 2)
    n = int(ep[-1])
    assert 100 < n < 130 * 100
    kid = MEASURES.index(measure)
    cols = _device_columns(torch, *S.pack_strings(Q), *S.pack_strings(Cs))
    # exact, guard elements behind both outputs
    rc, nnz, indptr, index, dist = _raw_device_call(ctx, torch, kid, cols, len(Q), len(Cs), 2, 0, n, n + 16)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and np.array_equal(index[:n], ei) and np.array_equal(dist[:n], ed)
    assert (index[n:] == GUARD_I).all() and (dist[n:] == GUARD_D).all()
    # one less: indptr and nnz are still exact, not one element of the outputs is touched
    rc, nnz, indptr, index, dist = _raw_device_call(ctx, torch, kid, cols, len(Q), len(Cs), 2, 0, n - 1, n + 16)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and (index == GUARD_I).all() and (dist == GUARD_D).all()
    # count only: zero with NULL outputs
    rc, nnz, indptr, index, dist = _raw_device_call(ctx, torch, kid, cols, len(Q), len(Cs), 2, 0, 0, 8)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and (index == GUARD_I).all() and (dist == GUARD_D).all()
    # a capacity far above every possible hit is no reason for a buffer of that size
    rc, nnz, indptr, index, dist = _raw_device_call(ctx, torch, kid, cols, len(Q), len(Cs), 2, 1, 1 << 40, n)
    up = R.from_distances(M, 2, True)
    assert rc == 0 and nnz == up[1].size and np.array_equal(indptr, up[0]) and np.array_equal(index[:nnz], up[1]) and np.array_equal(dist[:nnz], up[2])
    # the binding's retry: a guess that is too small, then the exact size; and its count-only form
    _assert_same(_run(ctx, measure, Q, Cs, 2, capacity=3), (ep, ei, ed), "retry")
    assert np.array_equal(ctx.distance_join(measure, *S.pack_strings(Q), *S.pack_strings(Cs), 2, count_only=True), ep)


# ---- 5. relations to untouched kernels -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", MEASURES)
def test_distance_join_gpu_unbounded_equals_the_pairwise_call(ctx, measure):
    # the explicit cross product of a 65 x 65 corner through the pairwise distance call: every pair, the same d
    Q, Cs, M = F.geometry(measure, 65, 65)
    A = [s for s in Q for _ in Cs]
    B = Cs * len(Q)
    if measure == "damerau_levenshtein":
        P = ctx.damerau_distance_host(*S.pack_strings(A), *S.pack_strings(B))
    else:
        P = ctx.distance_host(measure, *S.pack_strings(A), *S.pack_strings(B))
    P = np.asarray(P).reshape(len(Q), len(Cs))
    assert np.array_equal(P, M)
    _assert_same(_run(ctx, measure, Q, Cs, None), R.from_distances(P, None), measure)
    _assert_same(_run(ctx, measure, Q, Cs, UNBOUNDED - 1), R.from_distances(P, None), measure + " at 2^32 - 2")
    _assert_same(_run(ctx, measure, Q, Cs, 2), R.from_distances(P, 2), measure + " at 2")


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_distance_join_gpu_hits_grow_from_levenshtein_to_osa_to_damerau(ctx, k):
    # dl <= osa <= lev: row by row the hits of one are a subset of the next one's
    X = list(F.near_duplicates())
    Q, Cs = list(F.boundary())
    for A, B in ((X[:257], X), (Q, Cs)):
        lev, osa, dl = (_run(ctx, m, A, B, k) for m in MEASURES)
        grown = 0
        for i in range(len(A)):
            hits = [set(g[1][int(g[0][i]):int(g[0][i + 1])].tolist()) for g in (lev, osa, dl)]
            assert hits[0] <= hits[1] <= hits[2], (k, i)
            grown += len(hits[2]) - len(hits[0])
        assert grown > 0 or k == 0
    # k = 0 is the exact-duplicate join by every measure
    if k == 0:
        assert R.same(lev, osa) and R.same(osa, dl)


# ---- 6. entry points -------------------------------------------------------------------------------------------------------------

def test_distance_join_gpu_launch_counts_and_the_other_joins(ctx):
    # a call enqueues what match_join enqueues and one finishing kernel when hits are stored; the existing families keep their counts
    torch = pytest.importorskip("torch")
    L = S.lib()
    X = F.near_duplicates()
    cols = _device_columns(torch, *S.pack_strings(X[:100]), *S.pack_strings(X[:90]))
    ops = lambda: L.strsim_ctx_enqueued_ops(ctx._h)
    for measure in MEASURES:
        ctx.synchronize()
        n0 = ops()
        ctx.distance_join(measure, *cols, 2, count_only=True)
        n1 = ops()
        ctx.distance_join(measure, *cols, 2, capacity=100 * 90)
        n2 = ops()
        ctx.synchronize()
        assert (n1 - n0, n2 - n1) == (16, 19), measure
    n0 = ops()
    ctx.match_join("levenshtein", *cols, 0.8, count_only=True)
    n1 = ops()
    ctx.qgram_join("sorensen_dice", *cols, 0.6, count_only=True)
    n2 = ops()
    ctx.join("indel", *cols, 0.8, count_only=True)
    assert (n1 - n0, n2 - n1) == (16, 16) and ops() - n2 > 0


def test_distance_join_gpu_device_and_host_entry_points_between_other_calls(ctx):
    torch = pytest.importorskip("torch")
    Q, Cs, M = F.geometry("damerau_levenshtein", 100, 90)
    exp = R.from_distances(M, 2)
    assert F.not_vacuous(M, 2)
    host = (*S.pack_strings(Q), *S.pack_strings(Cs))
    dev = _device_columns(torch, *host)
    before = ctx.pairs_host("levenshtein", *S.pack_strings(Q[:50]), *S.pack_strings(Cs[:50]))
    _assert_same(ctx.distance_join("damerau_levenshtein", *host, 2), exp, "host")
    mj = ctx.match_join("levenshtein", *host, 0.8)
    indptr, index, dist = ctx.distance_join("damerau_levenshtein", *dev, 2)
    ctx.synchronize()
    assert indptr.is_cuda and index.is_cuda and dist.is_cuda
    _assert_same((indptr.cpu().numpy().astype(np.uint64), index.cpu().numpy().view(np.uint32), dist.cpu().numpy().view(np.uint32)), exp, "device")
    lev = ctx.distance_join("levenshtein", *dev, 3)
    ctx.synchronize()
    _assert_same((lev[0].cpu().numpy().astype(np.uint64), lev[1].cpu().numpy().view(np.uint32), lev[2].cpu().numpy().view(np.uint32)),
                 R.from_distances(np.ascontiguousarray(F.near_matrix("levenshtein")[:100, :90]), 3), "levenshtein, device")
    _assert_same(ctx.distance_join("damerau_levenshtein", *host, 2), exp, "host again")
    # the calls around it give what they gave
    assert np.array_equal(ctx.pairs_host("levenshtein", *S.pack_strings(Q[:50]), *S.pack_strings(Cs[:50])).view(np.uint64), before.view(np.uint64))
    again = ctx.match_join("levenshtein", *host, 0.8)
    assert all(np.array_equal(a, b) for a, b in zip(mj, again)) and mj[1].size > 0


def test_distance_join_gpu_edge_shapes(ctx):
    for measure in MEASURES:
        for Q, Cs in (([], ["a"]), (["a"], []), ([], [])):
            indptr, index, dist = _run(ctx, measure, Q, Cs, 1)
            assert indptr.tolist() == [0] * (len(Q) + 1) and index.size == 0 and dist.size == 0
        _assert_same(_run(ctx, measure, ["", "a"], ["", "a", "b"], 0), R.join(measure, ["", "a"], ["", "a", "b"], 0), "empty strings")
        _assert_same(_run(ctx, measure, ["", ""], ["", "", ""], 0, True), R.join(measure, ["", ""], ["", "", ""], 0, True), "only empty strings")


# ---- 7. the Python surface -------------------------------------------------------------------------------------------------------

def test_distance_join_gpu_python_surface_nulls_and_dedupe(ctx):
    Q = ["night", None, "abc", "nigth"]
    Cs = [None, "night", "abc", None, "nacht", "nights"]
    indptr, index, dist = S.distance_join("osa", Q, Cs, 2, ctx=ctx)
    assert indptr.dtype == np.int64 and index.dtype == np.int64 and dist.dtype == np.uint32
    assert indptr.tolist() == [0, 3, 3, 4, 6] and index.tolist() == [1, 4, 5, 2, 1, 5] and dist.tolist() == [0, 2, 1, 0, 1, 2]
    assert S.distance_join("levenshtein", Q, Cs, 1, ctx=ctx)[1].tolist() == [1, 5, 2]
    assert S.distance_join("osa", ["Night!"], ["night"], 0, ctx=ctx, processor="default_process")[2].tolist() == [0]
    X = list(F.near_duplicates()[:80])
    M = np.ascontiguousarray(F.near_matrix("damerau_levenshtein")[:80, :80])
    ep, ei, ed = R.from_distances(M, 2, True)
    assert 0 < ei.size
    i, j, d = S.distance_dedupe_pairs("damerau_levenshtein", X, 2, ctx=ctx)
    assert np.array_equal(i, np.repeat(np.arange(80), np.diff(ep.astype(np.int64)))) and np.array_equal(j, ei.astype(np.int64))
    assert np.array_equal(d, ed) and d.dtype == np.uint32
    with pytest.raises(ValueError, match="unknown edit distance"):
        S.distance_join("ratio", Q, Cs, 1, ctx=ctx)


def test_distance_join_gpu_fallback_leaves_last_wave_rows_alone(ctx):
    # the fallback's internal pairwise calls do not change what strsim_ctx_last_wave_rows reports of the caller's own last call
    A, B = ["müller", "abc", "x" * 70], ["muller", "abd", "x" * 69]
    ctx.damerau_distance_host(*S.pack_strings(A), *S.pack_strings(B))
    assert ctx.last_wave_rows == 2
    Q, Cs = ["night", "müller", "a" * 40], ["nacht", "night", "muller", "a" * 41, "日本"]
    for measure in MEASURES:
        for k in (1, 3, None):
            _assert_same(_run(ctx, measure, Q, Cs, k), R.join(measure, Q, Cs, k), "slow on both sides")
    assert ctx.last_wave_rows == 2
