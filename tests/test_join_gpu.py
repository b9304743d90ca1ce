"""Threshold join on the MI355X (strsim_join_*) against the contract stated independently (tests/join_ref.py): a brute force over
the pairwise scores of the models the searches are tested against.  Everything is compared exactly: indptr, the candidate indices
in ascending order, and the scores bit for bit."""
import ctypes as C
import functools
import math
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import extract_ref
import gen
import indel_ref
import join_ref as R

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polars-strsim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness", "join_harness.cpp")
INF = float("inf")
GUARD_I = 0x5EA1F00D
GUARD_S = 0x7FF8C0FFEE15BAD1  # a NaN payload no score has


def E(d, s):
    return indel_ref.normalise(d, s, 0)


# none, 0, 0.5, E(2, 6) and its two f64 neighbours, 1.0 and 1.5
CUTS = (None, 0.0, 0.5, math.nextafter(E(2, 6), 0.0), E(2, 6), math.nextafter(E(2, 6), 2.0), 1.0, 1.5)


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def H():
    """the host rules of strsim_join.h (the split rule, the sort's tier limit)"""
    d = tempfile.TemporaryDirectory(prefix="join_harness_")
    so = os.path.join(d.name, "libjoin_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", CSRC, "-fPIC", "-shared", "-o", so, HARNESS])
    L = C.CDLL(so)
    L.join_splits_h.restype = C.c_uint32
    L.join_splits_h.argtypes = [C.c_uint64, C.c_uint64, C.c_int]
    L.join_sort_wave_max.restype = C.c_uint32
    yield L
    d.cleanup()


def _run(ctx, scorer, Q, Cs, cut=None, upper=False, **kw):
    qo, qv = S.pack_strings(Q)
    co, cv = S.pack_strings(Cs)
    got = ctx.join(R.MEASURE[scorer], qo, qv, co, cv, cut, upper, **kw)
    assert got[0].shape == (len(Q) + 1,) and got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float64
    return got


def _assert_same(got, exp, what=""):
    gp, gi, gs = got
    ep, ei, es = exp
    assert np.array_equal(gp.astype(np.uint64), ep), "%s: indptr differs, first row %d" % (what, int(np.flatnonzero(gp.astype(np.uint64) != ep)[0]))
    assert np.array_equal(gi, ei), "%s: indices differ" % what
    assert np.array_equal(np.ascontiguousarray(gs).view(np.uint64), es.view(np.uint64)), "%s: scores differ" % what


def _strings(seed, n, alphabet=gen.ASCII_LOWER, lo=0, hi=12):
    A, B = gen.pairs(seed, (n + 1) // 2, alphabet, lo, hi)
    return (A + B)[:n]


def _device_columns(torch, *cols):
    dev = torch.device("cuda", 0)
    out = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.uint8)).to(dev) for x in cols]
    torch.cuda.synchronize()
    return out


# ---- shapes -------------------------------------------------------------------------------------------------------------------

Q_ROWS = (0, 1, 63, 64, 65, 257)


def _split_rows(H):
    """a candidate count at which the split rule gives several splits for 257 queries on this device"""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    nc = 129
    assert H.join_splits_h(257, nc, cu) >= 2
    return nc


@functools.lru_cache(maxsize=None)
def _shape_frame(nc):
    Q = _strings(201, max(Q_ROWS), hi=9)
    Cs = _strings(202, nc, hi=9)
    M = extract_ref.score_matrix("ratio", Q, Cs)
    M.setflags(write=False)
    return Q, Cs, M


@pytest.mark.parametrize("upper", [False, True])
def test_join_gpu_shapes_and_cutoffs(ctx, H, upper):
    # a wave less a lane, exactly one, one more, more than a workgroup; no candidate, one, a few, and several splits
    nc = _split_rows(H)
    Q, Cs, M = _shape_frame(nc)
    for q in Q_ROWS:
        for c in (0, 1, 9, nc):
            for cut in CUTS:
                _assert_same(_run(ctx, "ratio", Q[:q], Cs[:c], cut, upper), R.from_scores(M[:q, :c], cut, upper), "%d x %d at %r" % (q, c, cut))


def test_join_gpu_without_a_cutoff_is_cdist_as_csr(ctx, H):
    Q, Cs, M = _shape_frame(_split_rows(H))
    for cut in (None, -INF, 0.0):
        indptr, index, score = _run(ctx, "ratio", Q[:65], Cs[:40], cut)
        assert np.array_equal(indptr, np.arange(66, dtype=np.uint64) * 40) and np.array_equal(index, np.tile(np.arange(40, dtype=np.uint32), 65))
        assert np.array_equal(score.view(np.uint64), np.ascontiguousarray(M[:65, :40]).reshape(-1).view(np.uint64))


@pytest.mark.parametrize("upper", [False, True])
def test_join_gpu_every_length(ctx, upper):
    # every length 0 .. 32 on both sides, two strings of each: the window's edges, the empty string against everything
    rng = random.Random(7)
    Q = ["".join(rng.choice("abc") for _ in range(n)) for n in range(33) for _ in range(2)]
    Cs = ["".join(rng.choice("abc") for _ in range(n)) for n in range(33) for _ in range(2)]
    M = extract_ref.score_matrix("ratio", Q, Cs)
    for cut in CUTS:
        _assert_same(_run(ctx, "ratio", Q, Cs, cut, upper), R.from_scores(M, cut, upper), "at %r" % (cut,))


def test_join_gpu_empty_strings(ctx):
    _assert_same(_run(ctx, "ratio", ["", ""], ["", "", ""], 1.0), R.join("ratio", ["", ""], ["", "", ""], 1.0))
    got = _run(ctx, "ratio", ["", "a"], ["", "a", "b"], 0.5)
    assert got[0].tolist() == [0, 1, 2] and got[1].tolist() == [0, 1] and got[2].tolist() == [1.0, 1.0]
    for Q, Cs in (([], ["a"]), (["a"], []), ([], [])):
        indptr, index, score = _run(ctx, "ratio", Q, Cs, 0.5)
        assert indptr.tolist() == [0] * (len(Q) + 1) and index.size == 0 and score.size == 0


# ---- strings outside the lane class -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", ["query", "candidate", "both"])
@pytest.mark.parametrize("cut", [None, 0.5])
@pytest.mark.parametrize("upper", [False, True])
def test_join_gpu_slow_strings(ctx, side, cut, upper):
    # a 33-byte ASCII string and a 2-byte-UTF-8 one go through the pairwise call; near copies of them are hits across the classes
    Q = _strings(211, 70)
    Cs = _strings(212, 37)
    long33 = "abcdefghij klmnopqrst uvwxyzabcde"[:33]
    assert len(long33.encode()) == 33
    if side in ("query", "both"):
        Q[33] = long33
        Cs[5] = long33[:32]
    if side in ("candidate", "both"):
        Cs[17] = "héllo wörld"
        Q[3] = "hello world"
    if side == "both":
        Q[64] = "ñandú"
        Cs[0] = "x" * 40
        Cs[36] = long33
        Q[69] = "x" * 39
    _assert_same(_run(ctx, "ratio", Q, Cs, cut, upper), R.join("ratio", Q, Cs, cut, upper), side)


@pytest.mark.parametrize("slow_side", ["queries", "candidates", "both"])
def test_join_gpu_no_fast_string_on_a_side(ctx, slow_side):
    fast = _strings(221, 20)
    slow = ["long string number %02d, well beyond the lane class" % i for i in range(7)] + ["żółć%d" % i for i in range(5)]
    Q = slow if slow_side in ("queries", "both") else fast
    Cs = slow[::-1] if slow_side in ("candidates", "both") else fast
    for cut in (None, 0.8):
        _assert_same(_run(ctx, "ratio", Q, Cs, cut), R.join("ratio", Q, Cs, cut), slow_side)


# ---- self-join ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_slow", [False, True])
def test_join_gpu_upper_self_join(ctx, with_slow):
    base = _strings(231, 40, hi=8)
    X = base + [s + "x" for s in base[:30]] + base[:20]
    if with_slow:
        X[7] = "a string of more than thirty-two bytes"
        X[50] = "a string of more than thirty-two bytez"
        X[60] = "naïve"
        X[80] = "naïve"
    M = extract_ref.score_matrix("ratio", X, X)
    for cut in (0.0, 0.8, 1.0):
        indptr, index, score = got = _run(ctx, "ratio", X, X, cut, True)
        _assert_same(got, R.from_scores(M, cut, True), "upper at %r" % cut)
        rows = np.repeat(np.arange(len(X)), np.diff(indptr).astype(np.int64))
        assert (rows < index).all()
        # (i, j) is present iff (j, i) would be: the full join holds both
        fp, fi, _ = _run(ctx, "ratio", X, X, cut, False)
        full = set(zip(np.repeat(np.arange(len(X)), np.diff(fp).astype(np.int64)).tolist(), fi.tolist()))
        pairs = set(zip(rows.tolist(), index.tolist()))
        assert pairs == {(i, j) for (i, j) in full if i < j} and all((j, i) in full for (i, j) in pairs)


# ---- the sort's tiers ---------------------------------------------------------------------------------------------------------

def test_join_gpu_sort_tiers(ctx, H):
    # duplicated candidates: rows of 0, 1, 2, 63, 64, 65, tier limit, tier limit + 1 and 3 x tier limit hits
    tier = H.join_sort_wave_max()
    sizes = [0, 1, 2, 63, 64, 65, tier, tier + 1, 3 * tier]
    names = ["name%02dzz" % k + "qrstuvwxyz"[k] * 4 for k in range(len(sizes))]
    Cs = [nm for nm, n in zip(names, sizes) for _ in range(n)] + _strings(241, 200, hi=6)
    random.Random(3).shuffle(Cs)
    for cut in (1.0, 0.95):
        indptr, index, score = got = _run(ctx, "ratio", names, Cs, cut)
        _assert_same(got, R.join("ratio", names, Cs, cut), "tiers at %r" % cut)
        assert np.diff(indptr).tolist() == sizes
    for i in range(len(names)):
        assert (np.diff(index[int(indptr[i]):int(indptr[i + 1])].astype(np.int64)) > 0).all()


# ---- capacity -----------------------------------------------------------------------------------------------------------------

def _raw_device_call(ctx, torch, cols, nq, nc, cut, flags, capacity, room):
    """strsim_join_device with guard values in every output; -> (rc, nnz, indptr, index raw, score raw as uint64)"""
    dev = cols[0].device
    indptr = torch.full((nq + 1,), -7, dtype=torch.int64, device=dev)
    index = torch.from_numpy(np.full(room, GUARD_I, dtype=np.uint32).view(np.int32)).to(dev)
    score = torch.from_numpy(np.full(room, GUARD_S, dtype=np.uint64).view(np.int64)).to(dev)
    nnz = C.c_uint64(123456789)
    rc = S.lib().strsim_join_device(ctx._h, 8, cols[0].data_ptr(), cols[1].data_ptr(), nq, cols[2].data_ptr(), cols[3].data_ptr(), nc, cut, flags,
                                    capacity, indptr.data_ptr(), index.data_ptr() if capacity else None, score.data_ptr() if capacity else None,
                                    C.byref(nnz))
    ctx.synchronize()
    return rc, nnz.value, indptr.cpu().numpy().astype(np.uint64), index.cpu().numpy().view(np.uint32), score.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("slow", [False, True])
def test_join_gpu_capacity_protocol(ctx, H, slow):
    torch = pytest.importorskip("torch")
    Q, Cs, M = _shape_frame(_split_rows(H))
    Q, Cs = list(Q[:130]), list(Cs[:100])
    if slow:
        Q[5] = "q" * 40
        Cs[9] = "çà et là"
    ep, ei, es = R.join("ratio", Q, Cs, 0.5)
    n = int(ep[-1])
    assert n > 100
    cols = _device_columns(torch, *S.pack_strings(Q), *S.pack_strings(Cs))
    # exact
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, cols, len(Q), len(Cs), 0.5, 0, n, n + 16)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and np.array_equal(index[:n], ei) and np.array_equal(score[:n], es.view(np.uint64))
    assert (index[n:] == GUARD_I).all() and (score[n:] == GUARD_S).all()
    # one less: indptr and nnz are still exact, not one element of the outputs is touched
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, cols, len(Q), len(Cs), 0.5, 0, n - 1, n + 16)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and (index == GUARD_I).all() and (score == GUARD_S).all()
    # count only: zero with NULL outputs
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, cols, len(Q), len(Cs), 0.5, 0, 0, 8)
    assert rc == 0 and nnz == n and np.array_equal(indptr, ep) and (index == GUARD_I).all() and (score == GUARD_S).all()
    # oversize: nothing is written past nnz
    rc, nnz, indptr, index, score = _raw_device_call(ctx, torch, cols, len(Q), len(Cs), 0.5, 0, 3 * n, 3 * n + 16)
    assert rc == 0 and nnz == n and np.array_equal(index[:n], ei) and np.array_equal(score[:n], es.view(np.uint64))
    assert (index[n:] == GUARD_I).all() and (score[n:] == GUARD_S).all()
    # the binding's retry: a guess that is too small, then the exact size
    _assert_same(_run(ctx, "ratio", Q, Cs, 0.5, capacity=3), (ep, ei, es), "retry")
    assert np.array_equal(ctx.join("indel", *S.pack_strings(Q), *S.pack_strings(Cs), 0.5, count_only=True), ep)


def test_join_gpu_device_columns_give_device_results(ctx, H):
    torch = pytest.importorskip("torch")
    Q, Cs, M = _shape_frame(_split_rows(H))
    cols = _device_columns(torch, *S.pack_strings(Q[:100]), *S.pack_strings(Cs[:90]))
    indptr, index, score = ctx.join("indel", *cols, 0.6)
    ctx.synchronize()
    assert indptr.is_cuda and index.is_cuda and score.is_cuda
    _assert_same((indptr.cpu().numpy().astype(np.uint64), index.cpu().numpy().view(np.uint32), score.cpu().numpy()), R.from_scores(M[:100, :90], 0.6), "device")


# ---- token_sort_ratio ---------------------------------------------------------------------------------------------------------

def test_join_gpu_token_sort_ratio(ctx):
    rng = random.Random(16)
    first = ["john", "mary", "ann", "li", "omar", "zoe"]
    last = ["smith", "jones", "wu", "garcia", "o neil"]
    people = ["%s %s" % (rng.choice(first), rng.choice(last)) for _ in range(60)]
    Q = ["smith john"] + people[:40] + ["", "  "]
    Cs = ["john  smith"] + [" ".join(reversed(p.split())) for p in people[20:]] + ["\tsmith\njohn ", ""]
    for cut in (None, 0.8, 1.0):
        for upper in (False, True):
            _assert_same(_run(ctx, "token_sort_ratio", Q, Cs, cut, upper), R.join("token_sort_ratio", Q, Cs, cut, upper), "at %r" % (cut,))
    indptr, index, score = _run(ctx, "token_sort_ratio", Q, Cs, 1.0)
    assert 0 in index[:int(indptr[1])].tolist() and score[0] == 1.0


# ---- a larger shape against the library's own cdist -------------------------------------------------------------------------------

def _near_duplicates(seed, cands, n, alphabet="abcdefghijklmnopqrstuvwxyz"):
    """bench_support/bench_nearest.py's generator: a candidate with up to three random edits"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = list(rng.choice(cands))
        for _ in range(rng.randint(0, 3)):
            op = rng.randrange(4)
            p = rng.randrange(len(s) + 1)
            if op == 0:
                s.insert(p, rng.choice(alphabet))
            elif op == 1 and s:
                del s[min(p, len(s) - 1)]
            elif op == 2 and s:
                s[min(p, len(s) - 1)] = rng.choice(alphabet)
            elif op == 3 and len(s) >= 2:
                p = min(p, len(s) - 2)
                s[p], s[p + 1] = s[p + 1], s[p]
        out.append("".join(s))
    return out


def test_join_gpu_equals_thresholded_cdist_at_a_larger_shape(ctx):
    # cdist is held to the model by its own tests; here it is the yardstick at a size the pure-Python model cannot reach
    Cs = _strings(251, 3000, lo=1, hi=32)
    Q = _near_duplicates(252, Cs, 2000)
    Q[17] = Q[17] + " and then a tail that takes it out of the lane class"
    qo, qv = S.pack_strings(Q)
    co, cv = S.pack_strings(Cs)
    M = ctx.cdist("indel", qo, qv, co, cv)
    for cut in (0.8, 0.9):
        got = ctx.join("indel", qo, qv, co, cv, cut)
        _assert_same(got, R.from_scores(M, cut), "2000 x 3000 at %r" % cut)
        assert int(got[0][-1]) >= 400  # (a quarter of the queries are exact copies)


def test_join_gpu_more_fallback_scores_than_the_count_pass_keeps(ctx):
    # 2 200 slow queries x 8 020 candidates are more than the 2^24 scores the count pass keeps: the fill walks the slow strings again
    rng = random.Random(5)
    base = ["customer record number %04d of the archive" % k for k in range(300)]
    Q = [rng.choice(base) for _ in range(2200)] + _strings(271, 40)
    Cs = _strings(272, 8000, lo=1, hi=20) + base[:20]
    assert 2200 * len(Cs) > 2 ** 24 and all(len(s) > 32 for s in base)
    qo, qv = S.pack_strings(Q)
    co, cv = S.pack_strings(Cs)
    M = ctx.cdist("indel", qo, qv, co, cv)
    got = ctx.join("indel", qo, qv, co, cv, 0.9)
    _assert_same(got, R.from_scores(M, 0.9), "2 240 x 8 020, the fallback twice")
    assert int(got[0][-1]) >= 2200 * 20 // 300


# ---- one context, many calls ----------------------------------------------------------------------------------------------------

def test_join_gpu_back_to_back_calls_reuse_the_scratch(ctx, H):
    Q, Cs, M = _shape_frame(_split_rows(H))
    for q, c in ((5, 7), (257, 129), (64, 9), (200, 100), (1, 129), (257, 1)):
        for cut in (0.4, 0.9):
            _assert_same(_run(ctx, "ratio", Q[:q], Cs[:c], cut), R.from_scores(M[:q, :c], cut), "%d x %d" % (q, c))


def test_join_gpu_launch_counts(ctx, H):
    # without slow strings: pack (4), the fallback list's clear, the length order (5), the count sweep, totals + scan (4) and the
    # nnz read-back; then the fill sweep and one sort launch (two when a row can exceed the wave tier)
    torch = pytest.importorskip("torch")
    L = S.lib()
    Q, Cs, M = _shape_frame(_split_rows(H))
    cols = _device_columns(torch, *S.pack_strings(Q[:100]), *S.pack_strings(Cs[:90]))
    ops = lambda: L.strsim_ctx_enqueued_ops(ctx._h)
    ctx.synchronize()
    n0 = ops()
    ctx.join("indel", *cols, 0.6, count_only=True)
    n1 = ops()
    ctx.join("indel", *cols, 0.6, capacity=100 * 90)
    n2 = ops()
    ctx.join("indel", *cols, 1.5)
    n3 = ops()
    ctx.synchronize()
    assert (n1 - n0, n2 - n1, n3 - n2) == (16, 18, 1)
    big = _device_columns(torch, *S.pack_strings(Q[:10]), *S.pack_strings(_strings(261, H.join_sort_wave_max() + 1, hi=5)))
    n4 = ops()
    ctx.join("indel", *big, 0.6, capacity=10 * 600)
    assert ops() - n4 == 19
    ctx.synchronize()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def test_join_gpu_python_surface_nulls_and_dedupe(ctx):
    Q = ["anna", None, "bob", "anne"]
    Cs = [None, "anna", "bob", None, "anne", "bobby"]
    indptr, index, score = S.join("ratio", Q, Cs, 0.7, ctx=ctx)
    assert indptr.dtype == np.int64 and index.dtype == np.int64 and score.dtype == np.float64
    assert indptr.tolist() == [0, 2, 2, 4, 6] and index.tolist() == [1, 4, 2, 5, 1, 4]
    assert score.tolist() == [1.0, E(2, 8), 1.0, E(2, 8), E(2, 8), 1.0]
    col = ["anna", "bob", None, "anna", "Anna ", "bob"]
    i, j, s = S.dedupe_pairs("ratio", col, 1.0, ctx=ctx)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 3), (1, 5)] and s.tolist() == [1.0, 1.0]
    i, j, s = S.dedupe_pairs("ratio", col, 1.0, ctx=ctx, processor="default_process")
    assert list(zip(i.tolist(), j.tolist())) == [(0, 3), (0, 4), (1, 5), (3, 4)]
    with pytest.raises(ValueError, match="no join by scorer"):
        S.join("jaro", Q, Cs, 0.5, ctx=ctx)
