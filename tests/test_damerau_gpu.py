"""Unrestricted Damerau-Levenshtein on the GPU against tests/damerau_ref.py (the full-matrix DP in C): f64 bit for bit, u32
exactly.  The known answers, the lane tier and its cut, the wave tier at the strip and LDS / scratch boundaries, everything in one
call under both context modes, literals, empty strings, zero rows, the cutoff, the metric and the order of the three edit distances
from the GPU's own numbers, and the device entry points."""
import random

import numpy as np
import pytest

import damerau_ref as R
import gen

pytestmark = pytest.mark.gpu
LANE_MAX = 32    # DL_LANE_MAX: both strings ASCII and at most this long take the lane tier
LDS_COLS = 2048  # DL_WAVE_LDS_COLS: beyond it the boundary row of the shorter string lives in the context's scratch
CUTOFFS = (0, 1, 2, 5, 40, None)


@pytest.fixture(scope="module")
def S():
    import strsim_amd
    return strsim_amd


@pytest.fixture(scope="module")
def ctx(S):
    with S.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def cref():
    return R.CRef()


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def sim(S, ctx, A, B):
    return ctx.damerau_host(*S.pack_strings(A), *S.pack_strings(B))


def dist(S, ctx, A, B, k=None):
    return ctx.damerau_distance_host(*S.pack_strings(A), *S.pack_strings(B), k)


def lane_row(a, b):
    a, b = a.encode(), b.encode()
    return len(a) <= LANE_MAX and len(b) <= LANE_MAX and max(a + b + b"\0") < 128


def check(S, ctx, cref, A, B, wave_rows=None, want=None):
    """the similarity bit for bit and the unbounded distance exactly, with the tier counter of either call"""
    d, s = want if want is not None else (cref.distances(A, B), cref.scores(A, B))
    got = sim(S, ctx, A, B)
    if wave_rows is not None:
        assert ctx.last_wave_rows == wave_rows
    bad = np.flatnonzero(bits(got) != bits(s))
    assert bad.size == 0, [(i, got[i], s[i]) for i in bad[:5]]
    got = dist(S, ctx, A, B)
    if wave_rows is not None:
        assert ctx.last_wave_rows == wave_rows
    bad = np.flatnonzero(got != d)
    assert bad.size == 0, [(i, got[i], d[i]) for i in bad[:5]]


def test_dl_gpu_known_answers(S, ctx):
    for a, b, d, _ in R.KNOWN:
        for x, y in ((a, b), (b, a)):
            want = R.normalise(d, len(a), len(b))
            assert sim(S, ctx, [x], [y])[0] == want, (x, y)
            assert S.damerau_levenshtein([x], [y], ctx=ctx)[0] == want, (x, y)
            assert S.damerau_levenshtein_distance([x], [y], ctx=ctx)[0] == d, (x, y)
    for a, b, s in R.KNOWN_SCORES:
        assert sim(S, ctx, [a], [b])[0] == s == sim(S, ctx, [b], [a])[0]
    A, B = [k[0] for k in R.KNOWN], [k[1] for k in R.KNOWN]
    assert list(dist(S, ctx, A + B, B + A)) == [k[2] for k in R.KNOWN] * 2
    # nulls propagate
    got = S.damerau_levenshtein(["ca", None, "x"], ["abc", "a", None], ctx=ctx)
    assert got[0] == R.score("ca", "abc") and np.isnan(got[1]) and np.isnan(got[2])
    got = S.damerau_levenshtein_distance(["ca", None, "x"], "abc", ctx=ctx)
    assert got[0] == 2 and list(got.mask) == [False, True, False]


# ---- frames: built once, shared, never changed ----

@pytest.fixture(scope="module")
def lane_frame(cref):
    A, B = R.lane_frame(random.Random(41), 20000, LANE_MAX)
    return A, B, (cref.distances(A, B), cref.scores(A, B))


def cut_frame():
    """lengths at LANE_MAX - 1, at it and one beyond, on either side; and one non-ASCII byte in a row of lane size"""
    rng = random.Random(8)
    A, B = [], []
    edge = (0, 1, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1)
    for la in edge:
        for lb in edge:
            a = gen.rand_string(rng, R.LOWER, la, la)
            A += [a, a]
            B += [gen.rand_string(rng, R.LOWER, lb, lb), R.gapped(rng, a + gen.rand_string(rng, R.LOWER, 40, 40), 2, R.LOWER)[:lb]]
    for n in (1, 2, 15, LANE_MAX - 2):
        s = gen.rand_string(rng, R.LOWER, n, n)
        A += [s + "é", s, "\x7f" + s, s[:n // 2] + "\u0080" + s[n // 2:]]
        B += [s + "e", "ñ" + s, s, R.swapped(rng, s, 1)]
    return A, B


def boundary_frame():
    """scalar-value counts at the strip boundaries with the gapped edit across them, one- and two-byte characters"""
    A, B = [], []
    for unit in ("abcdefgh", "éèüñабвг"):
        base = "".join(unit[i % 8] for i in range(140))
        for n in (63, 64, 65, 127, 128, 129):
            for i in (n - 2, n - 1):  # x y across values n - 1 | n and n | n + 1 (1-based)
                b = R.gapped_at(base, i, "q")
                A += [base[:n + 3], b[:n + 1], base[:n]]
                B += [b[:n + 4], base[:n], b[:n]]
    return A, B


def wave_frame():
    rng = random.Random(17)
    A, B = gen.pairs(31, 400, gen.MIXED, 0, 80)
    A2, B2 = gen.pairs(32, 150, "éèüñßабвг", 0, 70)  # two-byte characters only
    A, B = A + A2, B + B2
    for _ in range(150):  # ASCII beyond the lane tier
        a = gen.rand_string(rng, R.LOWER, 65, 200)
        A.append(a)
        B.append(R.swapped(rng, R.gapped(rng, a, 3, R.LOWER), 2))
    A2, B2 = boundary_frame()
    return A + A2, B + B2


def long_frame():
    """2 047 / 2 048 / 2 049 values on the shorter side, the gapped edit on those columns; and 5 000 against 4 990"""
    rng = random.Random(23)
    base = "".join(rng.choice("abcdefgh") for _ in range(LDS_COLS + 80))
    A, B = [], []
    for n in (LDS_COLS - 1, LDS_COLS, LDS_COLS + 1):
        for i in (LDS_COLS - 2, LDS_COLS - 1):
            A += [base[:n + 70], R.gapped_at(base, i, "é")[:n]]
            B += [R.gapped_at(base, i, "q")[:n], base[:n + 3]]
    a = "".join(rng.choice("abcdeé") for _ in range(5000))
    A.append(a)
    B.append(R.swapped(rng, R.gapped(rng, a, 20, "abcdeé"), 20)[:4990])
    return A, B


@pytest.fixture(scope="module")
def mixed_frame(cref, lane_frame):
    """every tier in one call, shuffled"""
    A, B = list(lane_frame[0][:3000]), list(lane_frame[1][:3000])
    for X, Y in (cut_frame(), wave_frame(), long_frame()):
        A, B = A + X, B + Y
    A, B = A + ["", "", "a", "é"], B + ["", "a", "", ""]
    order = list(range(len(A)))
    random.Random(3).shuffle(order)
    A, B = [A[i] for i in order], [B[i] for i in order]
    return A, B, (cref.distances(A, B), cref.scores(A, B))


# ---- the tiers ----

def test_dl_gpu_lane_tier(S, ctx, lane_frame):
    A, B, want = lane_frame
    check(S, ctx, None, A, B, wave_rows=0, want=want)


def test_dl_gpu_lane_cut(S, ctx, cref):
    A, B = cut_frame()
    slow = sum(not lane_row(a, b) for a, b in zip(A, B))
    assert 0 < slow < len(A)
    check(S, ctx, cref, A, B, wave_rows=slow)


def test_dl_gpu_wave_tier(S, ctx, cref):
    A, B = wave_frame()
    check(S, ctx, cref, A, B, wave_rows=sum(not lane_row(a, b) for a, b in zip(A, B)))


def test_dl_gpu_long_rows(S, ctx, cref):
    A, B = long_frame()
    check(S, ctx, cref, A, B, wave_rows=len(A))
    # (and a short call after the scratch has grown)
    check(S, ctx, cref, ["ca", "é" * 70], ["abc", "é" * 69 + "x"], wave_rows=1)


@pytest.mark.parametrize("ordered", [0, 1])
def test_dl_gpu_mixed_call_in_both_context_modes(S, mixed_frame, ordered):
    A, B, want = mixed_frame
    with S.Context(0) as c:
        c.set_stream_ordered(bool(ordered))
        check(S, c, None, A, B, wave_rows=sum(not lane_row(a, b) for a, b in zip(A, B)), want=want)
        # another measure on the same context before and after
        lev = c.pairs_host("levenshtein", *S.pack_strings(A[:500]), *S.pack_strings(B[:500]))
        check(S, c, None, A, B, want=want)
        assert np.array_equal(bits(lev), bits(c.pairs_host("levenshtein", *S.pack_strings(A[:500]), *S.pack_strings(B[:500]))))


def test_dl_gpu_literals_empty_strings_and_zero_rows(S, ctx, cref, lane_frame):
    X = list(lane_frame[0][:1500]) + wave_frame()[0][:300] + ["", ""]
    for lit in ("jonh", "", "a" * LANE_MAX, "the quick brown fox jumps over the lazy dog", "é", "日本語" * 30):
        for A, B in (([lit], X), (X, [lit])):
            n_wave = sum(not lane_row(a, b) for a, b in zip(A * len(X) if len(A) == 1 else A, B * len(X) if len(B) == 1 else B))
            check(S, ctx, cref, A, B, wave_rows=n_wave)
    E = [""] * 300
    check(S, ctx, cref, E, E, wave_rows=0)
    assert (sim(S, ctx, E, E) == 1.0).all() and (dist(S, ctx, E, X[:300], 3) == R.clamp(cref.distances(E, X[:300]), 3)).all()
    assert sim(S, ctx, [], []).size == 0 and dist(S, ctx, [], [], 2).size == 0
    assert sim(S, ctx, ["a"], []).size == 0 and dist(S, ctx, [], ["a"]).size == 0


# ---- the distance ----

@pytest.mark.parametrize("k", CUTOFFS, ids=lambda k: "unbounded" if k is None else "k%d" % k)
def test_dl_gpu_distance_cutoff(S, ctx, mixed_frame, k):
    A, B, (d, s) = mixed_frame
    got = dist(S, ctx, A, B, k)
    want = R.clamp(d, k)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (k, [(A[i], B[i], got[i], want[i]) for i in bad[:3]])
    if k is None:
        la = np.array([len(a) for a in A])
        lb = np.array([len(b) for b in B])
        norm = np.array([R.normalise(int(x), int(p), int(q)) for x, p, q in zip(got, la, lb)])
        assert np.array_equal(bits(norm), bits(sim(S, ctx, A, B)))
        assert (got >= np.abs(la - lb)).all()
        assert np.array_equal(got, dist(S, ctx, B, A))  # symmetric


def test_dl_gpu_is_a_metric_below_osa_below_levenshtein(S, ctx):
    rng = random.Random(5)
    A, B, Cc = [], [], []
    for r in range(5000):
        hi = 12 if r % 10 else 75  # (a tenth of the triples beyond the lane tier)
        a = gen.rand_string(rng, "abcd", 0, hi)
        b = R.swapped(rng, R.gapped(rng, a, rng.randrange(3), "abcd"), rng.randrange(2))
        c = R.gapped(rng, R.swapped(rng, b, rng.randrange(2)), rng.randrange(3), "abcd")
        A.append(a)
        B.append(b)
        Cc.append(c)
    ab, bc, ac = (dist(S, ctx, X, Y).astype(np.int64) for X, Y in ((A, B), (B, Cc), (A, Cc)))
    assert (ac <= ab + bc).all()
    for X, Y, d in ((A, B, ab), (B, Cc, bc), (A, Cc, ac)):
        lev = S.levenshtein_distance(X, Y, ctx=ctx).astype(np.int64)
        osa = S.osa_distance(X, Y, ctx=ctx).astype(np.int64)
        assert (lev >= osa).all() and (osa >= d).all()
        assert (osa > d).any()


# ---- the device entry points ----

def test_dl_gpu_device_entry_points(S, ctx, mixed_frame):
    import torch
    A, B, (d, s) = mixed_frame

    def dev(X):
        off, val = S.pack_strings(X)
        val = val if val.size else np.zeros(1, dtype=np.uint8)
        return torch.from_numpy(off.view(np.int32).copy()).cuda(), torch.from_numpy(val.copy()).cuda()

    ao, av = dev(A)
    bo, bv = dev(B)
    out = ctx.damerau_device(ao, av, bo, bv)
    ctx.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(s))
    assert ctx.last_wave_rows == sum(not lane_row(a, b) for a, b in zip(A, B))
    for k in (None, 2):
        out = ctx.damerau_distance_device(ao, av, bo, bv, k)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), R.clamp(d, k))
    lo, lv = dev(["jonh"])
    out = ctx.damerau_distance_device(lo, lv, bo, bv, 3)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.clamp(R.CRef().distances(["jonh"], B), 3))
