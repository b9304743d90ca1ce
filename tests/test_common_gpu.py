"""Hamming, prefix, postfix and LCSseq on the GPU against tests/common_ref.py (plain Python over str): the counts exactly, the
distances exactly under every cutoff of CUTOFFS, the f64 similarity bit for bit, all four kinds.  The known answers, the lane tier
and its cut, every dword boundary of the lane windows and every shift of the end alignment, the wave tier at its chunk edges with
1- to 4-byte characters, long rows, literals in both tiers, empty strings and zero rows, every class in one call, the relations
between the kinds and to the edit distances from the GPU's own numbers, the device entry points, and the fuzz script."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import common_ref as R
import gen

pytestmark = pytest.mark.gpu
LANE_MAX = 32       # COMMON_LANE_MAX: both strings ASCII and at most this long take the lane tier of the three positional kinds
LCS_LANE_MAX = 128  # INDEL_LANE_MAX_BYTES: the same for lcs_seq
CUTOFFS = (0, 1, 2, 5, 40, None)
POSITIONAL = ("hamming", "prefix", "postfix")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def lane_row(kind, a, b):
    a, b = a.encode(), b.encode()
    cap = LCS_LANE_MAX if kind == "lcs_seq" else LANE_MAX
    return len(a) <= cap and len(b) <= cap and max(a + b + b"\0") < 128


def wave_rows(kind, A, B):
    n = max(len(A), len(B)) if len(A) and len(B) else 0
    A, B = (A * n if len(A) == 1 else A), (B * n if len(B) == 1 else B)
    return sum(not lane_row(kind, a, b) for a, b in zip(A, B))


def reference(A, B):
    """{kind: (counts, distances, scores)}"""
    return {kind: R.frame(kind, A, B) for kind in R.KINDS}


def check(S, ctx, A, B, want=None, kinds=R.KINDS, cutoffs=CUTOFFS, tiers=True):
    """the three outputs of every kind, with the size of the work list after each call"""
    want = want or reference(A, B)
    pa, pb = S.pack_strings(A), S.pack_strings(B)
    for kind in kinds:
        c, d, s = want[kind]
        slow = wave_rows(kind, A, B) if tiers else None
        got = ctx.common_count_host(kind, *pa, *pb)
        assert not tiers or ctx.last_wave_rows == slow, (kind, ctx.last_wave_rows, slow)
        bad = np.flatnonzero(got != c)
        assert bad.size == 0, (kind, "count", [(int(i), int(got[i]), int(c[i])) for i in bad[:5]])
        for k in cutoffs:
            got = ctx.common_distance_host(kind, *pa, *pb, k)
            assert not tiers or ctx.last_wave_rows == slow, (kind, k, ctx.last_wave_rows, slow)
            bad = np.flatnonzero(got != R.clamp(d, k))
            assert bad.size == 0, (kind, "distance", k, [(int(i), int(got[i]), int(d[i])) for i in bad[:5]])
        got = ctx.common_host(kind, *pa, *pb)
        assert not tiers or ctx.last_wave_rows == slow, (kind, ctx.last_wave_rows, slow)
        bad = np.flatnonzero(bits(got) != bits(s))
        assert bad.size == 0, (kind, "similarity", [(int(i), got[i], s[i]) for i in bad[:5]])


def test_common_gpu_known_answers_nulls_and_pad(S, ctx):
    for kind, a, b, c in R.KNOWN:
        for x, y in ((a, b), (b, a)):
            assert getattr(S, kind + "_similarity")([x], [y], ctx=ctx)[0] == c, (kind, x, y)
            assert getattr(S, kind + "_distance")([x], [y], ctx=ctx)[0] == max(len(a), len(b)) - c, (kind, x, y)
            assert getattr(S, kind)([x], [y], ctx=ctx)[0] == R.score(kind, a, b), (kind, x, y)
    for kind, a, b, d in R.KNOWN_DISTANCES:
        assert getattr(S, kind + "_distance")([a], [b], ctx=ctx)[0] == d == getattr(S, kind + "_distance")([b], [a], ctx=ctx)[0]
    assert S.lcs_seq(["AGGTAB"], ["GXTXAYB"], ctx=ctx)[0] == 1.0 - 3.0 / 7.0
    A, B = [k[1] for k in R.KNOWN], [k[2] for k in R.KNOWN]
    check(S, ctx, A + B, B + A)
    # nulls propagate
    for kind in R.KINDS:
        got = getattr(S, kind)(["abc", None, "x"], ["abd", "a", None], ctx=ctx)
        assert got[0] == R.score(kind, "abc", "abd") and np.isnan(got[1]) and np.isnan(got[2])
        for fn, want in ((kind + "_distance", R.distance(kind, "abc", "abd")), (kind + "_similarity", R.count(kind, "abc", "abd"))):
            got = getattr(S, fn)(["abc", None, "x"], "abd", ctx=ctx)
            assert got[0] == want and list(got.mask) == [False, True, False]
    # pad=False: rows whose character counts differ are nulls, decided from the inputs
    A, B = ["karolin", "abc", "éa", "", "日本", None, "x" * 40], ["kathrin", "abcdef", "ea", "", "日本語", "a", "y" * 40]
    d = S.hamming_distance(A, B, pad=False, ctx=ctx)
    assert list(d.mask) == [False, True, False, False, True, True, False] and [int(d[i]) for i in (0, 2, 3, 6)] == [3, 1, 0, 40]
    c = S.hamming_similarity(A, B, pad=False, ctx=ctx)
    assert list(c.mask) == list(d.mask) and [int(c[i]) for i in (0, 2, 3, 6)] == [4, 1, 0, 0]
    s = S.hamming(A, B, pad=False, ctx=ctx)
    assert list(np.isnan(s)) == list(d.mask) and s[0] == 1.0 - 3.0 / 7.0 and s[3] == 1.0
    d = S.hamming_distance(A, "kathrin", max_distance=2, pad=False, ctx=ctx)
    assert list(d.mask) == [False, True, True, True, True, True, True] and d[0] == 3
    assert list(S.hamming_distance(A[:5], B[:5], ctx=ctx)) == [3, 3, 1, 0, 1]  # (padded, the default)


# ---- frames: built once, shared, never changed ----

@pytest.fixture(scope="module")
def lane_frame():
    A, B = R.lane_frame(random.Random(41), 20000, LANE_MAX)
    return A, B, reference(A, B)


def cut_frame():
    """lengths 0, 1, 31, 32 and 33 on either side; one non-ASCII byte in a row of lane size; a 0x7F"""
    rng = random.Random(8)
    A, B = [], []
    edge = (0, 1, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1)
    for la in edge:
        for lb in edge:
            a = gen.rand_string(rng, "abc", la, la)
            A += [a, a, a]
            B += [gen.rand_string(rng, "abc", lb, lb), (a + gen.rand_string(rng, "abc", 40, 40))[:lb],
                  (gen.rand_string(rng, "abc", 40, 40) + a)[-lb:] if lb else ""]
    for n in (1, 2, 15, LANE_MAX - 2, LANE_MAX - 1):
        s = gen.rand_string(rng, R.LOWER, n, n)
        A += [s + "é", s, "\x7f" + s, s + "\x7f", s[:n // 2] + "\u0080" + s[n // 2:], "é" + s]
        B += [s + "e", "ñ" + s, s, "x" + s + "\x7f", s, "è" + s]
    return A, B


def dword_frame():
    """lengths 3, 4, 5, 7, 8, 9 (and 31, 32) with the only difference at each byte position; the shorter string 0..8 bytes
    shorter at either end, which runs every shift of the end alignment"""
    A, B = [], []
    for n in (3, 4, 5, 7, 8, 9, 31, 32):
        base = "".join("abcdefgh"[i % 8] for i in range(n))
        for pos in range(n):
            other = base[:pos] + "Z" + base[pos + 1:]
            for diff in range(0, min(8, n) + 1):
                A += [base, base, other, other]
                B += [other[diff:], other[:n - diff], base[diff:], base[:n - diff]]
        for diff in range(0, min(8, n) + 1):  # and no difference at all
            A += [base, base]
            B += [base[diff:], base[:n - diff]]
    return A, B


ALPHABETS = ("abcdefgh", "éèüñабвг", "日本語€₭Ⴌ한글", "😀😁𝄞𝄢🙂🙃", "aé日😀bè€𝄞")


def edge_frame():
    """63, 64, 65, 127, 128, 129 characters over 1-, 2-, 3- and 4-byte alphabets and a mixed one (a 64-byte chunk edge falls inside
    a character), the single difference on either side of each edge, from the front and from the back; for Hamming one string over
    2-byte characters against the same positions over 1-byte ones with equal tails, so that the cursors drift by more than a chunk"""
    A, B = [], []
    for alphabet in ALPHABETS:
        base = "".join(alphabet[(i * 5 + i // 7) % len(alphabet)] for i in range(140))
        for n in (63, 64, 65, 127, 128, 129):
            for i in (n - 66, n - 65, n - 64, n - 2, n - 1, 0, 1, 15, 16, 17, 20, 21, 22, 31, 32, 33, 42, 43):
                if not 0 <= i < n:
                    continue
                x = base[:n]
                y = x[:i] + "Q" + x[i + 1:]  # one byte in the place of the character: every byte behind it moves
                z = x[:i] + (alphabet[0] if x[i] != alphabet[0] else alphabet[1]) + x[i + 1:]  # the same width: none moves
                A += [x, x, x + "tail", y[n // 3:], x]
                B += [y, y[:n - 1], y, x, z]
    for n in (63, 64, 65, 127, 128, 129, 200):
        A += ["a" * n + "xyz", "é" * n + "xyz", "ab" * n + "é" * 70 + "q", "日" * n + "a" * n]
        B += ["é" * n + "xyz", "😀" * n + "xyz", "ab" * n + "e" * 70 + "q", "a" * n + "a" * n]
    return A, B


def long_frame():
    """a long ASCII pair (5 000 bytes) and a long mixed one, differences spread over them and at both ends"""
    rng = random.Random(23)
    A, B = [], []
    for alphabet in ("abcde", "aé日😀b"):
        a = "".join(rng.choice(alphabet) for _ in range(5000))
        b = list(a)
        for _ in range(40):
            b[rng.randrange(100, 4900)] = "Z"
        b = "".join(b)
        A += [a, a, a, "x" + a[1:], a]
        B += [b, b[:4990], b[10:], a[:4999] + "y", a]
    return A, B


def wave_frame():
    rng = random.Random(17)
    A, B = gen.pairs(31, 300, gen.MIXED, 0, 80)
    for _ in range(100):  # ASCII beyond the lane tier of the positional kinds, and some beyond LCSseq's
        a = gen.rand_string(rng, R.LOWER, 33, 200)
        A.append(a)
        B.append(R.edited(rng, a, R.LOWER, rng.randint(0, 4)))
    return A, B


@pytest.fixture(scope="module")
def mixed_frame(lane_frame):
    """every class in one call, shuffled"""
    A, B = list(lane_frame[0][:2000]), list(lane_frame[1][:2000])
    for X, Y in (cut_frame(), dword_frame()[0:2], wave_frame(), (edge_frame()[0][::7], edge_frame()[1][::7]), (long_frame()[0][:2], long_frame()[1][:2])):
        A, B = A + list(X[:600]), B + list(Y[:600])
    A, B = A + ["", "", "a", "é"], B + ["", "a", "", ""]
    order = list(range(len(A)))
    random.Random(3).shuffle(order)
    A, B = [A[i] for i in order], [B[i] for i in order]
    return A, B, reference(A, B)


# ---- the tiers ----

def test_common_gpu_lane_tier(S, ctx, lane_frame):
    A, B, want = lane_frame
    assert all(wave_rows(kind, A, B) == 0 for kind in R.KINDS)
    check(S, ctx, A, B, want)


def test_common_gpu_lane_cut(S, ctx):
    A, B = cut_frame()
    slow = wave_rows("hamming", A, B)
    assert 0 < slow < len(A) and wave_rows("lcs_seq", A, B) < slow
    check(S, ctx, A, B)


def test_common_gpu_dword_boundaries_and_every_shift(S, ctx):
    A, B = dword_frame()
    assert wave_rows("postfix", A, B) == 0
    check(S, ctx, A, B, cutoffs=(0, 1, 5, None))
    check(S, ctx, B, A, cutoffs=(2,))


def test_common_gpu_wave_tier_at_the_chunk_edges(S, ctx):
    A, B = edge_frame()
    assert wave_rows("prefix", A, B) == len(A)
    check(S, ctx, A, B, cutoffs=(0, 1, 2, None))
    check(S, ctx, B, A, cutoffs=(5, 40))


def test_common_gpu_wave_tier_random(S, ctx):
    A, B = wave_frame()
    check(S, ctx, A, B)


def test_common_gpu_long_rows(S, ctx):
    A, B = long_frame()
    check(S, ctx, A, B, cutoffs=(0, 5, 40, None))
    check(S, ctx, ["ab", "é" * 70], ["abc", "é" * 69 + "x"])  # (and a short call after the long one)


@pytest.mark.parametrize("ordered", [0, 1])
def test_common_gpu_mixed_call_in_both_context_modes(S, mixed_frame, ordered):
    A, B, want = mixed_frame
    with S.Context(0) as c:
        c.set_stream_ordered(bool(ordered))
        check(S, c, A, B, want, cutoffs=(1, None))
        # another measure on the same context before and after
        lev = c.pairs_host("levenshtein", *S.pack_strings(A[:500]), *S.pack_strings(B[:500]))
        check(S, c, A, B, want, cutoffs=(2,), tiers=False)
        assert np.array_equal(bits(lev), bits(c.pairs_host("levenshtein", *S.pack_strings(A[:500]), *S.pack_strings(B[:500]))))


def test_common_gpu_literals_empty_strings_and_zero_rows(S, ctx, lane_frame):
    X = list(lane_frame[0][:300]) + wave_frame()[0][250:330] + edge_frame()[0][:20] + ["", ""]
    for lit in ("jonh", "", "a" * LANE_MAX, "the quick brown fox jumps over the lazy dog", "日本語" * 30, X[310]):
        check(S, ctx, [lit], X, cutoffs=(1, None))
        check(S, ctx, X, [lit], cutoffs=(5,))
    E = [""] * 300
    check(S, ctx, E, E)
    check(S, ctx, E, X[:300], cutoffs=(3, None))
    for kind in R.KINDS:
        assert (ctx.common_host(kind, *S.pack_strings(E), *S.pack_strings(E)) == 1.0).all()
        for A, B in (([], []), (["a"], []), ([], ["a"])):
            pa, pb = S.pack_strings(A), S.pack_strings(B)
            assert ctx.common_host(kind, *pa, *pb).size == 0 and ctx.common_count_host(kind, *pa, *pb).size == 0
            assert ctx.common_distance_host(kind, *pa, *pb, 2).size == 0


@pytest.mark.parametrize("k", CUTOFFS, ids=lambda k: "unbounded" if k is None else "k%d" % k)
def test_common_gpu_distance_cutoff(S, ctx, mixed_frame, k):
    A, B, want = mixed_frame
    pa, pb = S.pack_strings(A), S.pack_strings(B)
    for kind in R.KINDS:
        got = ctx.common_distance_host(kind, *pa, *pb, k)
        bad = np.flatnonzero(got != R.clamp(want[kind][1], k))
        assert bad.size == 0, (kind, k, [(A[i], B[i], int(got[i]), int(want[kind][1][i])) for i in bad[:3]])


# ---- relations, from the GPU's own numbers ----

@pytest.mark.parametrize("which", ["lane", "wave"])
def test_common_gpu_relations(S, ctx, lane_frame, which):
    if which == "lane":
        A, B = lane_frame[0][:6000], lane_frame[1][:6000]
    else:
        A, B = wave_frame()
        X, Y = edge_frame()
        A, B = A + X[::5], B + Y[::5]
    pa, pb = S.pack_strings(A), S.pack_strings(B)
    c = {kind: ctx.common_count_host(kind, *pa, *pb).astype(np.int64) for kind in R.KINDS}
    d = {kind: ctx.common_distance_host(kind, *pa, *pb).astype(np.int64) for kind in R.KINDS}
    la, lb = np.array([len(a) for a in A]), np.array([len(b) for b in B])
    assert (c["prefix"] <= c["hamming"]).all() and (c["hamming"] <= c["lcs_seq"]).all() and (c["postfix"] <= c["lcs_seq"]).all()
    assert (c["lcs_seq"] <= np.minimum(la, lb)).all()
    for kind in R.KINDS:
        assert np.array_equal(d[kind], np.maximum(la, lb) - c[kind])
        assert np.array_equal(c[kind], ctx.common_count_host(kind, *pb, *pa))  # symmetric
        assert np.array_equal(bits(ctx.common_host(kind, *pa, *pb)), bits(ctx.common_host(kind, *pb, *pa)))
    lev = np.asarray(S.levenshtein_distance(A, B, ctx=ctx)).astype(np.int64)
    indel = np.asarray(S.indel_distance(A, B, ctx=ctx)).astype(np.int64)
    assert (d["hamming"] >= lev).all() and (lev >= d["lcs_seq"]).all()
    assert np.array_equal(indel, la + lb - 2 * c["lcs_seq"])
    ra, rb = S.pack_strings([a[::-1] for a in A]), S.pack_strings([b[::-1] for b in B])
    assert np.array_equal(c["postfix"], ctx.common_count_host("prefix", *ra, *rb))
    assert np.array_equal(c["prefix"], ctx.common_count_host("postfix", *ra, *rb))
    assert (c["hamming"] > c["prefix"]).any() and (c["lcs_seq"] > c["hamming"]).any() and (c["postfix"] > 0).any()


# ---- the device entry points ----

def test_common_gpu_device_entry_points(S, ctx, mixed_frame):
    import torch
    A, B, want = mixed_frame

    def dev(X):
        off, val = S.pack_strings(X)
        val = val if val.size else np.zeros(1, dtype=np.uint8)
        return torch.from_numpy(off.view(np.int32).copy()).cuda(), torch.from_numpy(val.copy()).cuda()

    ao, av = dev(A)
    bo, bv = dev(B)
    n, pad = len(A), 16
    for kind in R.KINDS:
        c, d, s = want[kind]
        out = ctx.common_device(kind, ao, av, bo, bv)
        ctx.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(s))
        assert ctx.last_wave_rows == wave_rows(kind, A, B)
        out = ctx.common_count_device(kind, ao, av, bo, bv)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), c)
        for k in (None, 2):
            out = ctx.common_distance_device(kind, ao, av, bo, bv, k)
            ctx.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), R.clamp(d, k))
        # an output at an offset into a larger buffer: the neighbours stay untouched
        big = torch.full((n + 2 * pad,), -7, dtype=torch.int32, device="cuda")
        ctx.common_distance_device(kind, ao, av, bo, bv, 5, out=big[pad:pad + n])
        ctx.synchronize()
        host = big.cpu().numpy()
        assert (host[:pad] == -7).all() and (host[pad + n:] == -7).all()
        assert np.array_equal(host[pad:pad + n].view(np.uint32), R.clamp(d, 5))
        bigf = torch.full((n + 2 * pad,), -7.5, dtype=torch.float64, device="cuda")
        ctx.common_device(kind, ao, av, bo, bv, out=bigf[pad:pad + n])
        ctx.synchronize()
        host = bigf.cpu().numpy()
        assert (host[:pad] == -7.5).all() and (host[pad + n:] == -7.5).all() and np.array_equal(bits(host[pad:pad + n]), bits(s))
    lo, lv = dev(["jonh"])
    for kind in R.KINDS:
        out = ctx.common_distance_device(kind, lo, lv, bo, bv, 3)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), R.clamp(R.frame(kind, ["jonh"], B)[1], 3))
        out = ctx.common_count_device(kind, ao, av, lo, lv)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), R.counts(kind, A, ["jonh"]))


# ---- the fuzz script ----

def test_common_gpu_fuzz_script():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_common_gpu.py"), "40", "7"], capture_output=True, text=True)
    assert run.returncode == 0 and "fuzz_common ok: 40 frames" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
