"""Indel (LCS) similarity and distance (measure 8) on the GPU, bit for bit / integer for integer against tests/indel_ref.py: the
known answers, a 200 000-row mixed frame, every tier boundary in one call, literals, long strings, what is left for the second
kernel, the cutoff of the distance form, and the other measures on the same context."""
import random

import numpy as np
import pytest

import gen
import indel_ref as R

pytestmark = pytest.mark.gpu
U = R.UNBOUNDED
FULL_ASCII = "".join(chr(c) for c in range(1, 128))


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


def sim(S, ctx, A, B):
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    return ctx.pairs_host("indel", ao, av, bo, bv)


def dist(S, ctx, A, B, k=None):
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    return ctx.distance_host("indel", ao, av, bo, bv, k)


def bcast(A, B):
    n = max(len(A), len(B))
    return (A * n if len(A) == 1 and n != 1 else A), (B * n if len(B) == 1 and n != 1 else B)


def ref_distances(A, B, cref):
    A, B = bcast(A, B)
    return R.mixed_distances(A, B, cref, short=32)


def lens(A, B):
    A, B = bcast(A, B)
    return [len(a) for a in A], [len(b) for b in B]


def same_bits(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, [(int(i), float(got[i]), float(exp[i])) for i in bad[:8]]


def same_ints(got, exp):
    got, exp = np.asarray(got).astype(np.int64), np.asarray(exp).astype(np.int64)
    assert got.shape == exp.shape
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, [(int(i), int(got[i]), int(exp[i])) for i in bad[:8]]


def check_both(S, ctx, A, B, cref, ks=(None,)):
    """The similarity call and the distance call (each cutoff of ks) against the reference; returns the distances."""
    d = ref_distances(A, B, cref)
    la, lb = lens(A, B)
    same_bits(sim(S, ctx, A, B), R.scores_from_distances(d, la, lb))
    for k in ks:
        same_ints(dist(S, ctx, A, B, k), R.clamp_array(d, U if k is None else k))
    return d


def lane_row(a, b):
    """What k_indel_lane takes: both strings ASCII and at most 128 bytes."""
    return a.isascii() and b.isascii() and len(a) <= 128 and len(b) <= 128


def test_known_answers(S, ctx):
    A, B = [k[0] for k in R.KNOWN], [k[1] for k in R.KNOWN]
    exp = [R.normalise(k[3], len(k[0]), len(k[1])) for k in R.KNOWN]
    assert exp[0] == 0.5 and exp[1] == 0.75 and exp[7] == 0.0 and exp[8] == 0.0 and exp[9] == 1.0
    same_bits(sim(S, ctx, A, B), exp)
    same_bits(sim(S, ctx, B, A), exp)
    same_bits(S.indel(A, B, ctx=ctx), exp)
    same_bits(S.similarity("indel", A, B, ctx=ctx), exp)
    same_ints(dist(S, ctx, A, B), [k[3] for k in R.KNOWN])
    same_ints(S.indel_distance(A, B, ctx=ctx).filled(0), [k[3] for k in R.KNOWN])
    same_ints(S.distance("indel", A, B, 1, ctx=ctx).filled(0), [min(k[3], 2) for k in R.KNOWN])


def test_mixed_frame_of_200k_rows(S, ctx, cref):
    A, B = gen.pairs(801, 120_000, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(802, 50_000, FULL_ASCII, 0, 30)
    A3, B3 = gen.pairs(803, 30_000, gen.MIXED, 0, 30)
    A4, B4 = gen.pairs(804, 2_000, gen.ASCII_LOWER, 20, 128, max_bytes=128)
    A5, B5 = gen.pairs(805, 1_000, gen.MIXED, 0, 200)
    A, B = A + A2 + A3 + A4 + A5, B + B2 + B3 + B4 + B5
    A += ["", "", "x", "same string", "é"]
    B += ["", "x", "", "same string", "é"]
    idx = list(range(len(A)))
    random.Random(8).shuffle(idx)
    A, B = [A[i] for i in idx], [B[i] for i in idx]
    assert len(A) >= 200_000 and sum(a == b for a, b in zip(A, B)) > 1000 and sum(not a for a in A) > 100
    check_both(S, ctx, A, B, cref, ks=(None, 3))
    assert ctx.last_late_rows == 0 and ctx.last_long_rows == 0


def _near(rng, a, m, alphabet):
    """A string of m characters made from a: a few substitutions, then cut or padded."""
    t = list(a)
    for _ in range(rng.randint(0, 3)):
        if t:
            t[rng.randrange(len(t))] = rng.choice(alphabet)
    t = t[:m] + [rng.choice(alphabet) for _ in range(m - len(t))]
    return "".join(t)


BOUNDS = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]


def test_every_tier_boundary_in_one_call(S, ctx, cref):
    """Byte lengths 31/32/33 .. 127/128/129 on either side, shuffled so that waves mix the width classes; 2-byte characters at the
    same counts; and the wave tier's limits: 255/256/257 values (registers / LDS) and 2047/2048/2049 (LDS / scratch)."""
    rng = random.Random(128)
    A, B = [], []
    for la in BOUNDS:
        for lb in BOUNDS:
            for _ in range(3):
                a = "".join(rng.choice("abc") for _ in range(la))
                A.append(a)
                B.append(_near(rng, a, lb, "abc"))
    for n in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257):
        for m in (n - 1, n, n + 1):
            a = "".join(rng.choice("éüab") for _ in range(n))
            A.append(a)
            B.append(_near(rng, a, m, "éüab"))
    for n in (2047, 2048, 2049):
        for m in (n - 1, n, n + 2):
            a = "".join(rng.choice("ab中") for _ in range(n))
            A.append(a)
            B.append(_near(rng, a, m, "ab中"))
            A.append(_near(rng, a, m, "ab中"))
            B.append(a)
    A += ["a" * 63 + "xy", "a" * 31 + "xy" + "a" * 40, "a" * 95 + "xy" + "b" * 31]
    B += ["a" * 63 + "yx", "a" * 31 + "yx" + "a" * 40, "a" * 95 + "yx" + "b" * 31]
    idx = list(range(len(A)))
    rng.shuffle(idx)
    A, B = [A[i] for i in idx], [B[i] for i in idx]
    check_both(S, ctx, A, B, cref, ks=(None, 2))
    assert ctx.last_wave_rows == sum(not lane_row(a, b) for a, b in zip(A, B))
    same_bits(sim(S, ctx, B, A), sim(S, ctx, A, B))


@pytest.mark.parametrize("lit", ["", "phillips", "mülelr", "x" * 128, "ab" * 64 + "c", "y" * 33, "é" * 40, "ab" * 200, "\x00a"])
def test_literal_on_either_side(S, ctx, cref, lit):
    A, B = gen.pairs(88, 3000, gen.MIXED, 0, 70)
    A2, B2 = gen.pairs(89, 3000, gen.ASCII_LOWER, 0, 128)
    A, B = A + A2, B + B2
    A[0], A[1], B[2] = "", "", ""
    check_both(S, ctx, A, [lit], cref, ks=(None, 16))
    slow = len(A) if not lane_row(lit, "") else sum(not lane_row(a, "") for a in A)
    assert ctx.last_wave_rows == slow
    check_both(S, ctx, [lit], B, cref, ks=(None, 16))


def test_small_shapes_and_errors(S, ctx):
    same_bits(sim(S, ctx, ["", ""], ["", "a"]), [1.0, 0.0])
    same_bits(sim(S, ctx, ["a"], ["a"]), [1.0])
    same_ints(dist(S, ctx, ["a"], ["b"]), [2])
    assert sim(S, ctx, [], []).shape == (0,) and dist(S, ctx, [], []).shape == (0,)
    with pytest.raises(S.ShapeMismatch):
        sim(S, ctx, ["a", "b"], ["a", "b", "c"])
    with pytest.raises(S.ShapeMismatch):
        dist(S, ctx, ["a", "b"], ["a", "b", "c"])
    got = S.indel(["jonh", None, "ab"], ["john", "x", None], ctx=ctx)
    assert got[0] == 0.75 and np.isnan(got[1]) and np.isnan(got[2])


@pytest.mark.parametrize("n", [5000, 20000])
def test_long_strings(S, ctx, cref, n):
    rng = random.Random(n)
    al = "abcé中😀"
    a = "".join(rng.choice(al) for _ in range(n))
    b = gen.edit(rng, a, al, n // 50)
    A, B = [a, a, b[: n // 3], "q", a], [b, a[::-1][: n // 2], a, a, a]
    d = [cref.distance(x, y) for x, y in zip(A, B)]
    same_bits(sim(S, ctx, A, B), [R.normalise(v, len(x), len(y)) for v, x, y in zip(d, A, B)])
    same_ints(dist(S, ctx, A, B), d)
    same_ints(dist(S, ctx, A, B, 100), R.clamp_array(d, 100))
    assert ctx.last_wave_rows == len(A)


def test_nothing_left_behind_an_ascii_frame(S, ctx, cref):
    """Rows of up to 128 ASCII bytes never reach the one-pair-per-wave kernel; the others all do."""
    A, B = gen.pairs(128, 20_000, FULL_ASCII, 0, 128, max_bytes=128)
    A2, B2 = gen.pairs(129, 2_000, gen.ASCII_LOWER, 100, 128, max_bytes=128)
    A, B = A + A2, B + B2
    assert max(len(a) for a in A) == 128 and max(len(b) for b in B) == 128
    check_both(S, ctx, A, B, cref)
    sim(S, ctx, A, B)
    assert ctx.last_wave_rows == 0 and ctx.last_late_rows == 0 and ctx.last_long_rows == 0
    A3, B3 = gen.pairs(130, 3_000, gen.MIXED, 0, 100)
    A4, B4 = gen.pairs(131, 500, gen.ASCII_LOWER, 129, 300)
    Am, Bm = A + A3 + A4, B + B3 + B4
    idx = list(range(len(Am)))
    random.Random(3).shuffle(idx)
    Am, Bm = [Am[i] for i in idx], [Bm[i] for i in idx]
    d = ref_distances(Am, Bm, cref)
    la, lb = lens(Am, Bm)
    same_bits(sim(S, ctx, Am, Bm), R.scores_from_distances(d, la, lb))
    slow = sum(not lane_row(a, b) for a, b in zip(Am, Bm))
    assert slow > 1000 and ctx.last_wave_rows == slow


@pytest.mark.parametrize("k", [0, 1, 3, 16, None])
def test_cutoff(S, ctx, cref, k):
    A, B = gen.pairs(160 + (k or 0), 30_000, gen.ASCII_LOWER, 0, 40)
    A2, B2 = gen.pairs(170 + (k or 0), 3_000, gen.MIXED, 0, 150)
    A, B = A + A2, B + B2
    d = ref_distances(A, B, cref)
    exp = R.clamp_array(d, U if k is None else k)
    same_ints(dist(S, ctx, A, B, k), exp)
    same_ints(dist(S, ctx, B, A, k), exp)
    if k is not None:
        assert int(exp.max()) == k + 1 and (exp <= k).any()


def test_distance_and_similarity_agree_bit_for_bit(S, ctx):
    A, B = gen.pairs(50, 45_000, gen.ASCII_LOWER, 0, 64)
    A2, B2 = gen.pairs(51, 5_000, gen.MIXED, 0, 90)
    A, B = A + A2, B + B2
    d = dist(S, ctx, A, B)
    got = sim(S, ctx, A, B)
    same_bits(got, R.scores_from_distances(d, [len(a) for a in A], [len(b) for b in B]))
    same_bits(sim(S, ctx, B, A), got)


def test_other_measures_on_the_same_context(S, ctx, cref):
    """The Indel path shares the context's OSA work list and scratch: Levenshtein, OSA and their distances before and after it."""
    import distance_ref as D
    import oracle_lib as O
    import osa_ref
    A, B = gen.pairs(60, 4000, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(61, 400, gen.MIXED, 0, 90)
    A, B = A + A2 + ["ab" * 1500, "q" * 3000], B + B2 + ["ba" * 1500, "q" * 2999 + "é"]
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    short = slice(0, 4000)
    cd = D.CDist()
    exp_lev = O.batch_strings("levenshtein", A, B, 4)
    exp_osa = np.array(osa_ref.batch_numpy(A[short], B[short]).tolist() + [osa_ref.CRef().score(a, b) for a, b in zip(A[4000:], B[4000:])])
    exp_osa_d = [cd.distance("osa", a, b) for a, b in zip(A, B)]
    exp_indel = ref_distances(A, B, cref)

    def others():
        same_bits(ctx.pairs_host("levenshtein", ao, av, bo, bv), exp_lev)
        same_bits(ctx.pairs_host("osa", ao, av, bo, bv), exp_osa)
        same_ints(ctx.distance_host("osa", ao, av, bo, bv), exp_osa_d)

    others()
    same_ints(ctx.distance_host("indel", ao, av, bo, bv), exp_indel)
    same_bits(ctx.pairs_host("indel", ao, av, bo, bv), R.scores_from_distances(exp_indel, [len(a) for a in A], [len(b) for b in B]))
    others()
    same_ints(ctx.distance_host("indel", ao, av, bo, bv, 4), R.clamp_array(exp_indel, 4))


def test_device_calls(S):
    import torch
    A, B = gen.pairs(9, 50_000, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(10, 2000, gen.MIXED, 0, 30)
    A, B = A + A2, B + B2
    d = R.batch_numpy_distance(A, B)
    exp = R.scores_from_distances(d, [len(a) for a in A], [len(b) for b in B])
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
    for one_launch in (False, True):
        with S.Context(0, one_launch=one_launch) as c:
            for _ in range(2):
                out = c.pairs_device("indel", dev(ao), dev(av), dev(bo), dev(bv))
                torch.cuda.synchronize()
                c.synchronize()
                same_bits(out.cpu().numpy(), exp)
                assert c.last_late_rows == 0 and c.last_long_rows == 0 and c.last_wave_rows == 2000 - sum(
                    a.isascii() and b.isascii() for a, b in zip(A2, B2))
                od = c.distance_device("indel", dev(ao), dev(av), dev(bo), dev(bv), 5)
                torch.cuda.synchronize()
                same_ints(od.cpu().numpy().view(np.uint32), R.clamp_array(d, 5))
