"""Optimal string alignment (measure 6) on the GPU, bit for bit against tests/osa_ref.py: the known answers, both kernel tiers and
calls that mix them, the mask-word boundaries, UTF-8 of every width, long strings, literals, a 2 M-row frame and both context
modes."""
import random

import numpy as np
import pytest

import gen
import osa_ref as R

pytestmark = pytest.mark.gpu


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


def run(S, ctx, A, B):
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    return ctx.pairs_host("osa", ao, av, bo, bv)


def expect(A, B, cref=None):
    n = max(len(A), len(B))
    A = A * n if len(A) == 1 else A
    B = B * n if len(B) == 1 else B
    if cref is not None:
        return np.array([cref.score(a, b) for a, b in zip(A, B)], dtype=np.float64)
    return np.array([R.score(a, b) for a, b in zip(A, B)], dtype=np.float64)


def same(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, [(int(i), float(got[i]), float(exp[i])) for i in bad[:8]]


def swapped(rng, s, k):
    t = list(s)
    for _ in range(k):
        if len(t) >= 2:
            i = rng.randrange(len(t) - 1)
            t[i], t[i + 1] = t[i + 1], t[i]
    return "".join(t)


def test_known_answers(S, ctx):
    A = [k[0] for k in R.KNOWN]
    B = [k[1] for k in R.KNOWN]
    same(run(S, ctx, A, B), [k[4] for k in R.KNOWN])
    same(run(S, ctx, B, A), [k[4] for k in R.KNOWN])
    same(S.osa(A, B, ctx=ctx), [k[4] for k in R.KNOWN])
    same(S.similarity("osa", A, B, ctx=ctx), [k[4] for k in R.KNOWN])


def test_lane_tier_ascii_up_to_64_bytes(S, ctx):
    rng = random.Random(1)
    A, B = [], []
    for _ in range(20000):
        a = "".join(rng.choice("abcd") for _ in range(rng.randint(0, 64)))
        A.append(a)
        B.append(swapped(rng, a, rng.randint(0, 4))[: rng.randint(0, 64)])
    same(run(S, ctx, A, B), R.batch_numpy(A, B))
    assert ctx.last_late_rows == 0 and ctx.last_long_rows == 0


def test_wave_tier_and_mixed_call(S, ctx):
    rng = random.Random(2)
    A, B = gen.pairs(3, 3000, gen.MIXED, 0, 80)               # non-ASCII and longer than 64 bytes: the wave tier
    A2, B2 = gen.pairs(4, 3000, gen.ASCII_LOWER, 0, 40)       # the lane tier
    A3 = ["".join(rng.choice("xyz") for _ in range(rng.randint(65, 200))) for _ in range(300)]
    B3 = [swapped(rng, a, 5) for a in A3]                     # long ASCII: the wave tier
    A, B = A + A2 + A3, B + B2 + B3
    idx = list(range(len(A)))
    rng.shuffle(idx)
    A, B = [A[i] for i in idx], [B[i] for i in idx]
    same(run(S, ctx, A, B), expect(A, B))
    assert ctx.last_late_rows == 0


@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65])
def test_byte_boundaries(S, ctx, n):
    rng = random.Random(n)
    A, B = [], []
    for m in (n - 1, n, n + 1):
        for _ in range(40):
            a = "".join(rng.choice("ab") for _ in range(n))
            A.append(a)
            B.append(swapped(rng, a, rng.randint(1, 3))[:m] + "b" * max(0, m - n))
    A.append("a" * (n - 2) + "xy")
    B.append("a" * (n - 2) + "yx")
    same(run(S, ctx, A, B), expect(A, B))


@pytest.mark.parametrize("n", [64, 65, 128, 129])
def test_code_point_boundaries(S, ctx, n):
    rng = random.Random(100 + n)
    A, B = [], []
    for m in (n - 1, n, n + 1):
        for _ in range(20):
            a = "".join(rng.choice("éü") for _ in range(n))
            A.append(a)
            B.append((swapped(rng, a, rng.randint(1, 3)) + "é")[:m])
    same(run(S, ctx, A, B), expect(A, B))


def test_transpositions_across_every_word_boundary(S, ctx, cref):
    """A swap at pattern positions (64k - 1, 64k) for every k of a 600-character pattern, ASCII and not."""
    A, B = [], []
    for fill in ("a", "ä"):
        base = [fill] * 600
        for k in range(1, 10):
            p = list(base)
            p[64 * k - 1], p[64 * k] = "x", "y"
            q = list(base)
            q[64 * k - 1], q[64 * k] = "y", "x"
            A.append("".join(p))
            B.append("".join(q))
            A.append("".join(p[:64 * k + 1]))
            B.append("".join(q[:64 * k + 1]) + "z")
    same(run(S, ctx, A, B), expect(A, B, cref))


def test_utf8_widths(S, ctx):
    rng = random.Random(5)
    alph = {2: "éüßñ", 3: "中文字€", 4: "😀🎉🚀🧪"}
    A, B = [], []
    for w, al in alph.items():
        for _ in range(300):
            a = "".join(rng.choice(al + "ab") for _ in range(rng.randint(0, 90)))
            A.append(a)
            B.append(swapped(rng, a, rng.randint(0, 4)))
    A += ["müller", "a😀b", "😀🎉"]
    B += ["mülelr", "ab😀", "🎉😀"]
    same(run(S, ctx, A, B), expect(A, B))


@pytest.mark.parametrize("n", [1000, 5000, 70000])
def test_long_strings(S, ctx, cref, n):
    rng = random.Random(n)
    al = "abcé中😀"
    a = "".join(rng.choice(al) for _ in range(n))
    b = swapped(rng, a, n // 50)
    b = b[: n - 7] + "xyz"
    A, B = [a, a, b[: n // 3], "q"], [b, a[::-1][: n // 2], a, a]
    same(run(S, ctx, A, B), expect(A, B, cref))


def test_empty_strings_and_literals(S, ctx):
    A, B = gen.pairs(8, 3000, gen.MIXED, 0, 70)
    A[0], A[1], B[2] = "", "", ""
    for lit in ("", "phillips", "jonh", "mülelr", "x" * 64, "y" * 65, "é" * 40, "ab" * 200):
        same(run(S, ctx, A, [lit]), expect(A, [lit]))
        same(run(S, ctx, [lit], B), expect([lit], B))
    same(run(S, ctx, ["", ""], ["", "a"]), [1.0, 0.0])
    same(run(S, ctx, ["a"], ["a"]), [1.0])
    with pytest.raises(S.ShapeMismatch):
        run(S, ctx, ["a", "b"], ["a", "b", "c"])


def test_nulls_through_similarity(S, ctx):
    got = S.osa(["jonh", None, "ab"], ["john", "x", None], ctx=ctx)
    assert got[0] == 0.75 and np.isnan(got[1]) and np.isnan(got[2])


def test_two_million_rows(S, ctx):
    rng = np.random.default_rng(2024)
    n = 2_000_000
    alph = np.array(list("abcdeé"))
    la = rng.integers(0, 17, n)
    chars = alph[rng.integers(0, len(alph), (n, 16))]
    A = ["".join(chars[i, :la[i]]) for i in range(n)]
    sw = rng.integers(0, 15, n)
    B = []
    for i, a in enumerate(A):
        j = sw[i]
        B.append(a[:j] + a[j + 1:j + 2] + a[j:j + 1] + a[j + 2:] if j + 1 < len(a) else a + "d")
    same(run(S, ctx, A, B), R.batch_numpy(A, B))


def test_device_calls_in_both_context_modes(S):
    import torch
    A, B = gen.pairs(9, 50000, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(10, 2000, gen.MIXED, 0, 120)
    A, B = A + A2 + ["q" * 2000], B + B2 + ["q" * 1999 + "r"]
    exp = R.batch_numpy(A[:50000], B[:50000]).tolist() + expect(A[50000:], B[50000:]).tolist()
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
    for one_launch in (False, True):
        with S.Context(0, one_launch=one_launch) as c:
            assert c.stream_ordered == (not one_launch)
            for _ in range(3):  # (the later calls of a one-launch context are enqueued as such)
                out = c.pairs_device("osa", dev(ao), dev(av), dev(bo), dev(bv))
                torch.cuda.synchronize()
                c.synchronize()
                same(out.cpu().numpy(), exp)
                assert c.last_late_rows == 0 and c.last_long_rows == 0
                # the five measures still work on the same context behind an OSA call
                lev = c.pairs_host("levenshtein", ao, av, bo, bv)
                assert lev.shape == (len(A),)
