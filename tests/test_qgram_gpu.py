"""q-gram similarity on the GPU, bit for bit against tests/qgram_ref.py: the known answers, every tier and mask-width boundary in
one frame, what is left for the second kernel, long rows on either side of the table's LDS limit, q = 1 against the reference
measures, literals, row counts, the device entry point, and other measures on the same context."""
import itertools
import random

import numpy as np
import pytest

import gen
import qgram_ref as R

pytestmark = pytest.mark.gpu
KNOWN, KNOWN_ANY = R.KNOWN, R.KNOWN_ANY
CONFIGS = [(q, multiset) for q in (1, 2, 3) for multiset in (True, False)]
LDS_GRAMS = 2048  # QGRAM_WAVE_LDS_GRAMS: pairs of more grams (both strings together) keep their table in the context's scratch


@pytest.fixture(scope="module")
def S():
    import strsim_amd
    return strsim_amd


@pytest.fixture(scope="module")
def ctx(S):
    with S.Context(0) as c:
        yield c


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def run(S, ctx, kind, A, B, q, multiset):
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    return ctx.qgram_host(kind, ao, av, bo, bv, q, multiset)


def check(S, ctx, A, B, q, multiset, kinds=R.KINDS, wave_rows=None):
    for kind in kinds:
        got = run(S, ctx, kind, A, B, q, multiset)
        if wave_rows is not None:
            assert ctx.last_wave_rows == wave_rows, (kind, q, multiset)
        want = R.batch(kind, A, B, q, multiset)
        bad = np.flatnonzero(bits(got) != bits(want))
        AA, BB = (A * len(want) if len(A) == 1 else A), (B * len(want) if len(B) == 1 else B)
        assert bad.size == 0, (kind, q, multiset, [(AA[i], BB[i], got[i], want[i]) for i in bad[:5]])


def lane_row(a, b):
    a, b = a.encode(), b.encode()
    return len(a) <= 64 and len(b) <= 64 and max(a + b + b"\0") < 128


def test_qgram_gpu_known_answers(S, ctx):
    for a, b, q, multiset, _, scores in KNOWN:
        for kind, want in scores.items():
            assert run(S, ctx, kind, [a], [b], q, multiset)[0] == want, (a, b, q, multiset, kind)
    for a, b, q, want in KNOWN_ANY:
        for kind in R.KINDS:
            for multiset in (True, False):
                assert run(S, ctx, kind, [a], [b], q, multiset)[0] == want
    # every kind x mode x q over the known pairs, as one column (and its mirror)
    A = [k[0] for k in KNOWN] + [k[0] for k in KNOWN_ANY]
    B = [k[1] for k in KNOWN] + [k[1] for k in KNOWN_ANY]
    for q, multiset in CONFIGS:
        check(S, ctx, A + B, B + A, q, multiset)


@pytest.fixture(scope="module")
def boundary_frame():
    rng = random.Random(77)
    A, B = [], []

    def add(a, b):
        A.append(a)
        B.append(b)

    edge = [0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65]
    for la, lb in itertools.product(edge, edge):  # lengths 0..q+1 and the mask-width and tier edges, on either side
        for al in ("ab", "abcdefgh"):
            a = gen.rand_string(rng, al, la, la)
            add(a, gen.rand_string(rng, al, lb, lb))
            add(a, (a + gen.rand_string(rng, al, 64, 64))[:lb])  # a shared prefix: many common grams
    for s in ("", "a", "ab", "b", "ba"):  # a == b shorter than q, and unequal strings as short
        for t in ("", "a", "ab", "b", "ba"):
            add(s, t)
    add("a\0", "a\0\0")
    add("a\0\0", "a\0")
    add("\0", "\0\0")
    add("\0" * 5, "\0" * 3)
    add("ab\0ab", "ab")
    for s, t in (("né", "ne"), ("日本語", "日本"), ("a😀b😀a", "😀b😀"), ("éa" * 3, "aé" * 3), ("𝄞日é", "é日𝄞"), ("ü", "ü"), ("ü", "u"),
                 ("añb", "anb"), ("日本語日本語", "本語日")):  # 2-, 3- and 4-byte characters with grams that straddle them
        add(s, t)
        add(t, s + "x")
    for n in (1, 2, 5, 20, 31):  # byte length in the lane class, but non-ASCII
        add("é" * n, "e" * n)
        add("a" * n + "ñ", "a" * n)
    return A, B


@pytest.mark.parametrize("q,multiset", CONFIGS)
def test_qgram_gpu_boundaries_in_one_frame(S, ctx, boundary_frame, q, multiset):
    A, B = boundary_frame
    slow = sum(not lane_row(a, b) for a, b in zip(A, B))
    assert 0 < slow < len(A) < 5000
    check(S, ctx, A, B, q, multiset, wave_rows=slow)


@pytest.mark.parametrize("multiset", [True, False])
def test_qgram_gpu_runs_of_one_character(S, ctx, multiset):
    # "a" * i against "a" * j for all i, j in 0..64 at q = 1: in multiset mode every product na * nb <= 4096 of the cosine and its
    # square root, against numpy's correctly rounded sqrt and division
    I, J = np.meshgrid(np.arange(65), np.arange(65), indexing="ij")
    I, J = I.ravel(), J.ravel()
    A, B = ["a" * int(i) for i in I], ["a" * int(j) for j in J]
    got = run(S, ctx, "cosine", A, B, 1, multiset)
    assert ctx.last_wave_rows == 0
    na, nb = (I, J) if multiset else (np.minimum(I, 1), np.minimum(J, 1))
    isect = np.minimum(na, nb).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = isect / np.sqrt((na * nb).astype(np.float64))
    want[(na == 0) | (nb == 0)] = 0.0
    want[I == J] = 1.0
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, [(int(I[k]), int(J[k]), got[k], want[k]) for k in bad[:5]]
    check(S, ctx, A, B, 1, multiset)
    for q in (2, 3):
        check(S, ctx, A, B, q, multiset, kinds=("cosine", "jaccard"))


def test_qgram_gpu_what_is_left_behind(S, ctx):
    A, B = gen.pairs(5, 3000, gen.ASCII_LOWER, 0, 64, max_bytes=64)
    check(S, ctx, A, B, 2, True, kinds=("sorensen_dice",), wave_rows=0)
    A2, B2 = list(A), list(B)
    A2[1234] = "é" + A2[1234][:20]
    check(S, ctx, A2, B2, 2, True, kinds=("sorensen_dice",), wave_rows=1)
    A2[1234] = A[1234]
    B2[2999] = "x" * 65
    check(S, ctx, A2, B2, 3, False, kinds=("jaccard",), wave_rows=1)
    A2[0] = "日本"
    check(S, ctx, A2, B2, 1, True, kinds=("cosine",), wave_rows=2)


@pytest.fixture(scope="module")
def long_rows():
    rng = random.Random(3)
    many = "".join(chr(c) for c in range(0x100, 0x100 + 700)) + gen.ASCII_LOWER  # many distinct grams, 2-byte characters among them

    def distinct(n):
        return "".join(rng.choice(many) for _ in range(n))

    A, B = [], []
    for n in (200, 1024, 1025, 1500, 5000):
        a = distinct(n)
        b = list(a)
        for _ in range(n // 20):
            b[rng.randrange(n)] = rng.choice(many)
        A += [a, "ab" * (n // 2), distinct(n), "ab" * (n // 2)]
        B += ["".join(b), "ba" * (n // 2) + "b", distinct(n - 7), "ab" * (n // 4) + "c"]
    # 1 500 values against 500: under the table's LDS limit; 5 000 against 5 000: over it; and the limit itself from both sides
    A += [distinct(1500), distinct(LDS_GRAMS // 2 + 1), distinct(LDS_GRAMS // 2 + 2), "ab" * 600]
    B += [distinct(500), distinct(LDS_GRAMS // 2 + 1), distinct(LDS_GRAMS // 2 + 1), "ab" * 500]
    A += [distinct(5000), "a", distinct(3000), distinct(60)]  # very different lengths, and a short pair among the long ones
    B += ["xyz", distinct(4000), distinct(30), distinct(70)]
    return A, B


@pytest.mark.parametrize("q,multiset", CONFIGS)
def test_qgram_gpu_long_rows(S, ctx, long_rows, q, multiset):
    A, B = long_rows
    grams = [max(len(a) - q + 1, 0) + max(len(b) - q + 1, 0) for a, b in zip(A, B)]
    assert min(grams) < 256 and any(256 < g <= LDS_GRAMS for g in grams) and any(g > LDS_GRAMS for g in grams)
    if q == 2:
        assert LDS_GRAMS in grams and LDS_GRAMS + 1 in grams
    check(S, ctx, A, B, q, multiset, wave_rows=len(A))


@pytest.mark.parametrize("kind", ["jaccard", "sorensen_dice"])
def test_qgram_gpu_at_q1_is_the_reference_measure(S, ctx, kind):
    A, B = gen.pairs(41, 14000, gen.ASCII_LOWER, 0, 40)
    A2, B2 = gen.pairs(42, 6000, gen.MIXED, 0, 90)
    A, B = A + A2, B + B2
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    got = ctx.qgram_host(kind, ao, av, bo, bv, 1, True)
    want = ctx.pairs_host(kind, ao, av, bo, bv)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert len(A) == 20000 and bad.size == 0, [(A[i], B[i], got[i], want[i]) for i in bad[:5]]


@pytest.mark.parametrize("q,multiset", CONFIGS)
def test_qgram_gpu_literals(S, ctx, q, multiset):
    col, _ = gen.pairs(51, 400, gen.ASCII_LOWER, 0, 64, max_bytes=64)
    col2, _ = gen.pairs(52, 150, gen.MIXED, 0, 40)
    col = col + col2 + ["", "a", "ab", "x" * 64, "x" * 65]
    slow = sum(not lane_row(c, "") for c in col)
    for lit, all_wave in (("", False), ("a", False), ("ab", False), ("night", False), ("né", True), ("ab" * 33, True), ("x" * 64, False)):
        kinds = R.KINDS if lit in ("night", "né") else ("sorensen_dice", "cosine")
        check(S, ctx, [lit], col, q, multiset, kinds=kinds, wave_rows=len(col) if all_wave else slow)
        check(S, ctx, col, [lit], q, multiset, kinds=kinds, wave_rows=len(col) if all_wave else slow)


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 4097])
def test_qgram_gpu_row_counts(S, ctx, rows):
    A, B = gen.pairs(60 + rows, rows, "abcé", 0, 70)
    for q, multiset in ((2, True), (3, False)):
        got = run(S, ctx, "jaccard", A, B, q, multiset)
        assert got.shape == (rows,)
        assert np.array_equal(bits(got), bits(R.batch("jaccard", A, B, q, multiset)))


def test_qgram_gpu_device_entry_point(S, ctx):
    import torch
    A, B = gen.pairs(71, 1500, gen.ASCII_LOWER, 0, 64, max_bytes=64)
    A2, B2 = gen.pairs(72, 200, gen.MIXED, 0, 90)
    A, B = A + A2 + ["ab" * 1200], B + B2 + ["ba" * 1300]
    slow = sum(not lane_row(a, b) for a, b in zip(A, B))
    dev = torch.device("cuda", 0)

    def to_dev(X):
        o, v = S.pack_strings(X)
        return torch.from_numpy(o.view(np.int32)).to(dev), torch.from_numpy(np.concatenate([v, np.zeros(1, np.uint8)])).to(dev)

    ao, av = to_dev(A)
    bo, bv = to_dev(B)
    lo, lv = to_dev(["night"])
    for kind, q, multiset in (("jaccard", 2, True), ("sorensen_dice", 3, True), ("overlap", 2, False), ("cosine", 1, False)):
        out = ctx.qgram_device(kind, ao, av, bo, bv, q, multiset)
        assert ctx.last_wave_rows == slow
        ctx.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(R.batch(kind, A, B, q, multiset)))
        out = ctx.qgram_device(kind, lo, lv, bo, bv, q, multiset)  # a literal, into a tensor of the caller's
        out2 = torch.full((len(B),), -1.0, dtype=torch.float64, device=dev)
        assert ctx.qgram_device(kind, bo, bv, lo, lv, q, multiset, out=out2) is out2
        ctx.synchronize()
        want = R.batch(kind, ["night"], B, q, multiset)
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)) and np.array_equal(bits(out2.cpu().numpy()), bits(want))
    with pytest.raises(S.ShapeMismatch):
        ctx.qgram_device("jaccard", ao, av, bo[:100], bv, 2, True)


def test_qgram_gpu_back_to_back_and_between_other_measures(S):
    import oracle_lib as O
    A, B = gen.pairs(81, 3000, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(82, 300, gen.MIXED, 0, 80)
    A, B = A + A2, B + B2
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    slow = sum(not lane_row(a, b) for a, b in zip(A, B))
    with S.Context(0) as c:
        lev = O.batch_strings("levenshtein", A, B, 4)
        first = c.pairs_host("levenshtein", ao, av, bo, bv)
        g1 = c.qgram_host("sorensen_dice", ao, av, bo, bv, 2, True)
        g2 = c.qgram_host("cosine", ao, av, bo, bv, 3, False)
        assert c.last_wave_rows == slow
        ind = c.pairs_host("indel", ao, av, bo, bv)
        g3 = c.qgram_host("sorensen_dice", ao, av, bo, bv, 2, True)
        last = c.pairs_host("levenshtein", ao, av, bo, bv)
        ind2 = c.pairs_host("indel", ao, av, bo, bv)
    assert np.array_equal(bits(first), bits(lev)) and np.array_equal(bits(last), bits(lev)) and np.array_equal(bits(ind), bits(ind2))
    assert np.array_equal(bits(g1), bits(R.batch("sorensen_dice", A, B, 2, True))) and np.array_equal(bits(g1), bits(g3))
    assert np.array_equal(bits(g2), bits(R.batch("cosine", A, B, 3, False)))


def test_qgram_gpu_helper_with_nulls(S, ctx):
    A = ["night", None, "abab", "", None]
    B = ["nacht", "x", None, "", None]
    got = S.qgram("jaccard", A, B, q=2, ctx=ctx)
    assert np.array_equal(np.isnan(got), [False, True, True, False, True]) and got[0] == 1 / 7 and got[3] == 1.0
    got = S.qgram("sorensen_dice", A, "abab", q=2, multiset=False, ctx=ctx)
    assert np.array_equal(np.isnan(got), [False, True, False, False, True]) and got[2] == 1.0 and got[3] == 0.0
    assert np.isnan(S.qgram("cosine", A, None, ctx=ctx)).all()
