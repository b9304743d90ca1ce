"""Bounded edit distances (strsim_distance_device / _host) on the GPU, exactly against tests/distance_ref.py for Levenshtein and OSA:
both kernel tiers, the mask-word boundaries and the LDS-to-scratch switch, UTF-8 of every width, 70 000-character strings with and
without a cutoff, literals, zero rows, the device and host entry points, the cutoff law on a 1 M-row frame and the tie to the
normalised similarities of strsim_pairs_device."""
import random

import numpy as np
import pytest

import distance_ref as R
import gen

pytestmark = pytest.mark.gpu
U = R.UNBOUNDED
MEASURES = ("levenshtein", "osa")


@pytest.fixture(scope="module")
def S():
    import strsim_amd
    return strsim_amd


@pytest.fixture(scope="module")
def ctx(S):
    with S.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def cdist():
    return R.CDist()


def run(S, ctx, measure, A, B, k=None):
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    return ctx.distance_host(measure, ao, av, bo, bv, k)


def _edits(rng, s, alphabet, n):
    t = list(s)
    for _ in range(n):
        op = rng.randrange(4)
        if op == 0 and t:
            t[rng.randrange(len(t))] = rng.choice(alphabet)
        elif op == 1:
            t.insert(rng.randint(0, len(t)), rng.choice(alphabet))
        elif op == 2 and t:
            del t[rng.randrange(len(t))]
        elif op == 3 and len(t) >= 2:
            i = rng.randrange(len(t) - 1)
            t[i], t[i + 1] = t[i + 1], t[i]
    return "".join(t)


@pytest.mark.parametrize("measure", MEASURES)
def test_dist_gpu_known_answers(S, ctx, measure):
    A = [k[0] for k in R.KNOWN]
    B = [k[1] for k in R.KNOWN]
    want = [k[2] if measure == "levenshtein" else k[3] for k in R.KNOWN]
    assert run(S, ctx, measure, A, B).tolist() == want
    assert run(S, ctx, measure, B, A).tolist() == want
    assert run(S, ctx, measure, A, B, 1).tolist() == [min(w, 2) for w in want]


@pytest.mark.parametrize("measure", MEASURES)
def test_dist_gpu_lane_tier_random_ascii(S, ctx, measure):
    rng = random.Random(1)
    A, B = [], []
    for _ in range(3000):
        a = gen.rand_string(rng, rng.choice(["ab", "abcd", gen.ASCII_LOWER]), 0, 64)
        b = _edits(rng, a, "abcd", rng.randint(0, 6)) if rng.random() < 0.7 else gen.rand_string(rng, "abcd", 0, 64)
        A.append(a)
        B.append(b[:64])
    full = R.batch_numpy(measure, A, B)
    for k in (None, 0, 1, 2, 10, 64):
        got = run(S, ctx, measure, A, B, k)
        want = full if k is None else np.minimum(full, k + 1)
        assert got.dtype == np.uint32 and np.array_equal(got, want), k


@pytest.mark.parametrize("measure", MEASURES)
def test_dist_gpu_wave_tier_word_boundaries(S, ctx, cdist, measure):
    """Scalar-value lengths around 64, 128 and the LDS limit of 2048 (beyond it the pattern lives in scratch)."""
    rng = random.Random(2)
    lens = (63, 64, 65, 127, 128, 129, 2047, 2048, 2049)
    A, B = [], []
    for la in lens:
        for lb in lens:
            if abs(la - lb) > 200:
                continue
            alphabet = rng.choice(["ab", "aé", "xyz東"])
            a = "".join(rng.choice(alphabet) for _ in range(la))
            near = (_edits(rng, a, alphabet, rng.randint(0, 8)) + "".join(rng.choice(alphabet) for _ in range(lb)))[:lb]
            far = "".join(rng.choice(alphabet) for _ in range(lb))
            A += [a, a]
            B += [near, far]
    full = [cdist.distance(measure, a, b) for a, b in zip(A, B)]
    for k in (None, 0, 3, 40, 100, 3000):
        got = run(S, ctx, measure, A, B, k).tolist()
        assert got == [R.clamp(d, k) for d in full], k


@pytest.mark.parametrize("measure", MEASURES)
def test_dist_gpu_every_utf8_width(S, ctx, cdist, measure):
    rng = random.Random(3)
    alphabet = "aZ" + "éß" + "日本" + "😀𝄞"  # 1, 2, 3 and 4 bytes
    A, B = [], []
    for _ in range(1500):
        a = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 100)))
        A.append(a)
        B.append(_edits(rng, a, alphabet, rng.randint(0, 10)) if rng.random() < 0.8 else
                 "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 100))))
    full = [cdist.distance(measure, a, b) for a, b in zip(A, B)]
    for k in (None, 0, 2, 7):
        assert run(S, ctx, measure, A, B, k).tolist() == [R.clamp(d, k) for d in full], k


@pytest.mark.parametrize("measure", MEASURES)
def test_dist_gpu_70000_characters(S, ctx, cdist, measure):
    rng = random.Random(4)
    alphabet = "abcdefghé日😀"
    a = "".join(rng.choice(alphabet) for _ in range(70000))
    near = _edits(rng, a, alphabet, 40)
    far = "".join(rng.choice("klmnop") for _ in range(69990))  # no character in common: d = max of the lengths
    d_near = cdist.distance(measure, a, near, band=400)
    A, B = [a, a, far], [near, far, a]
    for k in (0, 1, 5, 100, None):
        got = run(S, ctx, measure, A, B, k).tolist()
        assert got == [R.clamp(d_near, k), R.clamp(70000, k), R.clamp(70000, k)], k


@pytest.mark.parametrize("measure", MEASURES)
def test_dist_gpu_literal_either_side(S, ctx, measure):
    rng = random.Random(5)
    col = [gen.rand_string(rng, gen.MIXED, 0, 90) for _ in range(700)]
    for lit in ("", "abc", "héllo wörld", "x" * 70, "日本語" * 30):
        want = [R.distance(measure, lit, c) for c in col]
        for k in (None, 3):
            w = [R.clamp(d, k) for d in want]
            assert run(S, ctx, measure, [lit], col, k).tolist() == w
            assert run(S, ctx, measure, col, [lit], k).tolist() == w


def test_dist_gpu_zero_rows(S, ctx):
    for m in MEASURES:
        assert run(S, ctx, m, [], [], 3).size == 0
        assert run(S, ctx, m, ["abc"], [], None).size == 0


def test_dist_gpu_device_and_host_agree(S, ctx):
    import torch
    A, B = gen.pairs(11, 20000, gen.MIXED, 0, 150)
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev)
         for x in (ao, av if av.size else np.zeros(1, np.uint8), bo, bv if bv.size else np.zeros(1, np.uint8))]
    torch.cuda.synchronize()  # (the uploads ran on torch's stream, the distances run on the context's)
    for m in MEASURES:
        for k in (None, 0, 4):
            d = ctx.distance_device(m, t[0], t[1], t[2], t[3], k)
            ctx.synchronize()
            got = d.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, ctx.distance_host(m, ao, av, bo, bv, k)), (m, k)


def test_dist_gpu_cutoff_law_on_a_mixed_frame(S, ctx):
    """out(k) == min(out(unbounded), k + 1) on every row of a 1 M-row frame of both tiers."""
    A0, B0 = gen.pairs(12, 1 << 15, gen.MIXED, 0, 100)
    pick = np.random.default_rng(12).integers(0, len(A0), 1 << 20)  # (1 M rows drawn from 32 768 generated pairs)
    A, B = [A0[i] for i in pick], [B0[i] for i in pick]
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    for m in MEASURES:
        full = ctx.distance_host(m, ao, av, bo, bv)
        for k in (0, 1, 3, 8, 40):
            got = ctx.distance_host(m, ao, av, bo, bv, k)
            assert np.array_equal(got, np.minimum(full, k + 1)), (m, k)


def test_dist_gpu_matches_the_similarities(S, ctx):
    """1 - d / max(|a|, |b|) (1.0 for two empty strings) is bit for bit strsim_pairs_device's score, measures 0 and 6."""
    A, B = gen.pairs(13, 50000, gen.MIXED, 0, 120)
    A += ["", "", "abc", "a" * 3000]
    B += ["", "x", "abc", "a" * 2999 + "b"]
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    la = np.array([len(s) for s in A], dtype=np.float64)
    lb = np.array([len(s) for s in B], dtype=np.float64)
    for m in MEASURES:
        d = ctx.distance_host(m, ao, av, bo, bv).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = 1.0 - d / np.maximum(la, lb)
        want[(la == 0) & (lb == 0)] = 1.0
        sim = ctx.pairs_host(m, ao, av, bo, bv)
        assert np.array_equal(want.view(np.uint64), sim.view(np.uint64)), m


def _osa_tier_frame():
    """A few hundred pairs on every path of k_dist_lane / k_dist_wave: ASCII patterns (the longer string of a lane pair) of 0, 1,
    31..33 and 63, 64 bytes, 65-byte pairs (the first wave rows), short non-ASCII pairs, wave patterns (the string with fewer
    scalar values) of 64, 65 and 128 values, 2048 and 2049 values (the last pattern in LDS, the first in scratch), and swaps of two
    neighbours across byte 31/32 of a lane pair and across value 63/64 of a wave pair."""
    rng = random.Random(21)
    abc = "abcdefghijklmnopqrstuvwxyz"
    A, B = [], []
    for n in (0, 1, 31, 32, 33, 63, 64):
        for _ in range(12):
            a = "".join(rng.choice(abc) for _ in range(n))
            A += [a, a, a, a[: n // 2]]
            B += [_edits(rng, a, abc, rng.randint(0, 4))[:n], "".join(rng.choice(abc) for _ in range(rng.randint(0, n))), "", a]
    for _ in range(20):
        a = "".join(rng.choice(abc) for _ in range(65))
        A += [a, a[:40]]
        B += [(_edits(rng, a, abc, 5) + "xx")[:65], a]
    for _ in range(30):
        a = gen.rand_string(rng, gen.MIXED, 0, 20)
        A += [a, a]
        B += [_edits(rng, a, "é日😀ab", 3), gen.rand_string(rng, gen.MIXED, 0, 20)]
    for n in (64, 65, 128):
        for alphabet in (abc, "аб日😀éxyz"):
            for _ in range(4):
                a = "".join(rng.choice(alphabet) for _ in range(n))
                A += [a, a + "tail of the text"]
                B += [_edits(rng, a, alphabet, 6) + "longer", _edits(rng, a, alphabet, 3)[:n]]
    for n in (2048, 2049):
        a = "".join(rng.choice(abc) for _ in range(n))
        A.append(a)
        B.append(_edits(rng, a, abc, 40) + "z" * 50)
    for at, n in ((31, 40), (31, 64), (63, 70), (63, 200)):
        a = list("".join(rng.choice(abc) for _ in range(n)))
        a[at], a[at + 1] = "Q", "R"
        b = a[:]
        b[at], b[at + 1] = "R", "Q"
        A += ["".join(a), "".join(b)]
        B += ["".join(b), "".join(a) + ("é" if n > 64 else "")]
    assert 300 <= len(A) == len(B) <= 900
    return A, B


@pytest.fixture(scope="module")
def osa_tier_frame():
    return _osa_tier_frame()


@pytest.mark.parametrize("shape", ("rows", "literal a", "literal b"))
def test_dist_gpu_osa_similarity_is_the_epilogue_of_the_distance(S, ctx, osa_tier_frame, shape):
    """The OSA similarity and the OSA distance are two instantiations of one kernel pair: on the device, the similarity is bit for
    bit 1 - d / max(|a|, |b|) of the unbounded distance (1.0 for two empty strings), row against row and with a literal on either
    side."""
    import torch
    A, B = osa_tier_frame
    dev = torch.device("cuda", 0)

    def column(X):
        o, v = S.pack_strings(X)
        return [torch.from_numpy(o.view(np.int32)).to(dev), torch.from_numpy(v if v.size else np.zeros(1, np.uint8)).to(dev)]

    lits = ("", "a" * 31 + "QR" + "b" * 7, "héllo wörld", "x" * 70)
    cases = [(A, B)] if shape == "rows" else [([lit], B) if shape == "literal a" else (A, [lit]) for lit in lits]
    for X, Y in cases:
        cols = column(X) + column(Y)
        torch.cuda.synchronize()  # (the uploads ran on torch's stream, the calls run on the context's)
        d = ctx.distance_device("osa", *cols, None)
        sim = ctx.pairs_device("osa", *cols)
        ctx.synchronize()
        d = d.cpu().numpy().view(np.uint32).astype(np.float64)
        n = max(len(X), len(Y))
        la = np.array([len(s) for s in X], dtype=np.float64) * np.ones(n)
        lb = np.array([len(s) for s in Y], dtype=np.float64) * np.ones(n)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = 1.0 - d / np.maximum(la, lb)
        want[(la == 0) & (lb == 0)] = 1.0
        bad = np.flatnonzero(want.view(np.uint64) != sim.cpu().numpy().view(np.uint64))
        assert bad.size == 0, (shape, X[0][:20] if len(X) == 1 else Y[0][:20], bad[:5].tolist())


def test_dist_gpu_python_wrappers_mask_nulls(S):
    got = S.levenshtein_distance(["kitten", None, "abcd"], ["sitting", "x", "acbd"])
    assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.uint32
    assert got.mask.tolist() == [False, True, False] and got[0] == 3 and got[2] == 2
    got = S.osa_distance(["abcd", "ca"], "acbd", max_distance=1)
    assert got.tolist() == [1, 2]
    assert S.osa_distance(["abcd"], None).mask.tolist() == [True]
