"""Partial ratio (measure 10) on the GPU through the C ABI, bit for bit (== on the f64 bits) and integer for integer against the
brute-force model of tests/partial_ref.py: the headline frame, ties, equal lengths, every class boundary, non-ASCII rows, literals,
nulls, empty strings, small calls and scratch reuse."""
import random

import numpy as np
import pytest

import gen
import partial_ref as R

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


def bcast(A, B):
    n = max(len(A), len(B))
    return (A * n if len(A) == 1 and n != 1 else A), (B * n if len(B) == 1 and n != 1 else B)


def same_bits(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, (bad.size, [(int(i), float(got[i]), float(exp[i])) for i in bad[:8]])


def same_spans(got, exp):
    got, exp = np.asarray(got).astype(np.int64), np.asarray(exp).astype(np.int64)
    assert got.shape == exp.shape
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, (bad.size, [(int(i), got[i].tolist(), exp[i].tolist()) for i in bad[:8]])


def device_calls(S, ctx, A, B):
    """(score of strsim_pairs_device, score and span of strsim_partial_alignment_device) on device-resident columns."""
    import torch
    dev = torch.device("cuda", 0)

    def up(x):
        o, v = S.pack_strings(x)
        v = v if v.size else np.zeros(1, dtype=np.uint8)
        return torch.from_numpy(o.astype(np.int32)).to(dev), torch.from_numpy(v).to(dev)
    ao, av = up(A)
    bo, bv = up(B)
    torch.cuda.synchronize()
    s1 = ctx.pairs_device("partial_ratio", ao, av, bo, bv)
    ctx.synchronize()
    wave_rows = ctx.last_wave_rows
    s2, sp = ctx.partial_alignment_device(ao, av, bo, bv)
    ctx.synchronize()
    return s1.cpu().numpy(), s2.cpu().numpy(), sp.cpu().numpy().view(np.uint32), wave_rows


def check(S, ctx, cref, A, B, device=True):
    """Every entry point against the model; returns (the model's outputs, last_wave_rows of the device pairwise call)."""
    RA, RB = bcast(A, B)
    exp_s, exp_sp, ties, flag = cref.batch(RA, RB)
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    same_bits(ctx.pairs_host("partial_ratio", ao, av, bo, bv), exp_s)
    hs, hsp = ctx.partial_alignment_host(ao, av, bo, bv)
    same_bits(hs, exp_s)
    same_spans(hsp, exp_sp)
    wave_rows = None
    if device:
        s1, s2, sp, wave_rows = device_calls(S, ctx, A, B)
        same_bits(s1, exp_s)
        same_bits(s2, exp_s)
        same_spans(sp, exp_sp)
    return (exp_s, exp_sp, ties, flag), wave_rows


def test_partial_known_answers_on_the_gpu(S, ctx, cref):
    A, B = [k[0] for k in R.KNOWN], [k[1] for k in R.KNOWN]
    (s, sp, _, _), _ = check(S, ctx, cref, A, B)
    assert s.tolist() == [k[2] for k in R.KNOWN]
    assert sp.tolist() == [list(k[3] + k[4]) for k in R.KNOWN]
    check(S, ctx, cref, B, A)
    same_bits(S.partial_ratio(A, B, ctx=ctx), s)
    sc, span = S.partial_ratio_alignment(A, B, ctx=ctx)
    same_bits(sc, s)
    assert not span.mask.any() and span.filled(0).tolist() == sp.tolist()


def test_nothing_left_behind_on_the_headline_frame(S, ctx, cref):
    """200 000 rows U{1..32} lowercase ASCII: 0 mismatches, and no row goes to the wave kernel."""
    A, B = gen.pairs(1001, 200_000, gen.ASCII_LOWER, 1, 32, p_edit=0.0, p_same=0.0)  # (independent strings: both lengths U{1..32})
    assert max(map(len, A)) == 32 and max(map(len, B)) == 32 and min(map(len, A + B)) == 1
    _, wave_rows = check(S, ctx, cref, A, B)
    assert wave_rows == 0


def test_ties_two_letter_alphabet(S, ctx, cref):
    """50 000 rows over {a, b}, lengths 1..32, score and span.  The frame must exercise the tie rule: at least a quarter of its
    rows have more than one window at the maximum according to the model."""
    A, B = gen.pairs(1002, 50_000, "ab", 1, 32, p_edit=0.0, p_same=0.0)
    (_, _, ties, _), _ = check(S, ctx, cref, A, B)
    share = float((ties > 1).mean())
    print("rows with more than one window at the maximum: %.3f" % share)
    assert share >= 0.25


def test_equal_lengths_both_directions(S, ctx, cref):
    """5 000 rows with |a| = |b|.  At least a fifth must be rows where b as the needle is strictly better."""
    rng = random.Random(1003)
    A, B = [], []
    for r in range(5_000):
        n = rng.randint(1, 32)
        alphabet = ("ab", "abcd", "abcdefgh", gen.ASCII_LOWER)[r & 3]
        A.append("".join(rng.choice(alphabet) for _ in range(n)))
        B.append("".join(rng.choice(alphabet) for _ in range(n)))
    (_, _, _, flag), wave_rows = check(S, ctx, cref, A, B)
    share = float(flag.mean())
    print("rows where P(b, a) > P(a, b): %.3f" % share)
    assert share >= 0.2 and wave_rows == 0
    # the same through the wave tier: one non-ASCII character on both sides keeps the lengths equal
    A2, B2 = [a + "é" for a in A[:1500]], [b + "ü" for b in B[:1500]]
    (_, _, _, flag2), wave_rows2 = check(S, ctx, cref, A2, B2)
    assert wave_rows2 == 1500 and flag2.mean() >= 0.2


def test_class_boundaries(S, ctx, cref):
    """Lengths 31 / 32 / 33 on either side (32 bytes is the lane class's limit for the needle and the haystack alike), needles of
    63 / 64 / 65 and 128 / 129 / 130 values against haystacks of up to 1 000, and tables beyond the wave tier's LDS (16 KB: a
    haystack of more than 2 048 values for a short needle, 70 x 4 100 for a long one).  Rows with needles over 64 values are kept
    to a few dozen: the wave tier walks their windows one after the other, O(n m ceil(m / 64)) word steps a pair."""
    rng = random.Random(1004)

    def rs(n, alphabet="abc"):
        return "".join(rng.choice(alphabet) for _ in range(n))

    def planted(m, n):
        s = rs(m)
        k = rng.randrange(0, n - m + 1)
        t = rs(k) + s[:m // 2] + "#" + s[m // 2 + 1:] + rs(n - m - k)
        return s, t
    A, B = [], []
    for la in (0, 1, 2, 30, 31, 32, 33, 34):
        for lb in (0, 1, 2, 30, 31, 32, 33, 34, 64, 65):
            for _ in range(3):
                A.append(rs(la)); B.append(rs(lb))
    lane_rows = sum(1 for a, b in zip(A, B) if len(a) <= 32 and len(b) <= 32)
    for m in (63, 64, 65):
        for n in (m, m + 1, 127, 128, 129, 400, 1000):
            for _ in range(2):
                s, t = planted(m, n)
                A.append(s); B.append(t)
                A.append(t); B.append(s)
    long_needles = 0
    for m in (128, 129, 130):
        for n in (m, m + 1, 300, 1000):
            s, t = planted(m, n)
            A.append(s); B.append(t)
            long_needles += 1
    s, t = planted(12, 3000)  # the 64-bit table in the scratch
    A.append(s); B.append(t)
    A.append(t); B.append(s)
    s, t = planted(70, 4100)  # the word form in the scratch
    A.append(s); B.append(t)
    long_needles += 1
    assert long_needles <= 36
    _, wave_rows = check(S, ctx, cref, A, B)
    assert wave_rows == len(A) - lane_rows
    # scratch reuse: the same call again on the same context, then a call that needs none
    check(S, ctx, cref, A[-3:], B[-3:])
    check(S, ctx, cref, A[:50], B[:50])


def test_non_ascii_spans_are_in_scalar_values(S, ctx, cref):
    A, B = gen.pairs(1005, 20_000, gen.MIXED, 0, 30)
    A += ["müller", "日本", "😀x😀"]
    B += ["herr mülelr, k.", "これは日本語です", "ab😀x😀cd"]
    (s, sp, _, _), wave_rows = check(S, ctx, cref, A, B)
    assert sp[-3].tolist() == [0, 6, 5, 11] and s[-3] == 0.8333333333333334
    assert sp[-2].tolist() == [0, 2, 3, 5] and s[-2] == 1.0   # (bytes would be 9..15)
    assert sp[-1].tolist() == [0, 3, 2, 5] and s[-1] == 1.0
    assert wave_rows == sum(1 for a, b in zip(A, B) if not (a.isascii() and b.isascii()))


@pytest.mark.parametrize("literal", ["", "jon", "jonathan smith", "a" * 32, "a" * 33, "jonathan smith of rotterdam and of elsewhere", "müller"])
def test_literal_on_either_side(S, ctx, cref, literal):
    A, _ = gen.pairs(1006, 3_000, gen.ASCII_LOWER, 0, 32)
    A += ["", "jonathan smith", "jon", "müller strasse", "x" * 40]
    check(S, ctx, cref, A, [literal])
    check(S, ctx, cref, [literal], A)


def test_empty_strings_nulls_and_zero_rows(S, ctx, cref):
    A = ["", "", "abc", "", "x"]
    B = ["", "abc", "", "é", ""]
    (s, sp, _, _), _ = check(S, ctx, cref, A, B)
    assert s.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and not sp.any()
    check(S, ctx, cref, [""], [""])
    sc, span = S.partial_ratio_alignment(["abcd", None, "x", None], ["XXabcdXX", "y", None, None], ctx=ctx)
    assert sc[0] == 1.0 and np.isnan(sc[1:]).all()
    assert span[0].tolist() == [0, 4, 2, 6] and span.mask[1:].all() and not span.mask[0].any()
    one = S.partial_ratio(["abcd", None], ["XXabcdXX", "y"], ctx=ctx)
    assert one[0] == 1.0 and np.isnan(one[1])
    z = np.zeros(1, dtype=np.uint32)
    assert ctx.pairs_host("partial_ratio", z, np.zeros(1, np.uint8), z, np.zeros(1, np.uint8)).size == 0
    zs, zsp = ctx.partial_alignment_host(z, np.zeros(1, np.uint8), z, np.zeros(1, np.uint8))
    assert zs.size == 0 and zsp.shape == (0, 4)
    with pytest.raises(S.ShapeMismatch):
        ctx.partial_alignment_host(*S.pack_strings(["a", "b"]), *S.pack_strings(["a", "b", "c"]))


def test_small_device_call_and_back_to_back_calls(S, ctx, cref):
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    A, B = gen.pairs(1007, 700, gen.MIXED, 0, 40)
    exp_s, exp_sp, _, _ = cref.batch(A, B)
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    t = [torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev) for x in (ao, av, bo, bv)]
    out = torch.empty(len(A), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    L = S.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.strsim_pairs_device_small.restype = C.c_int
    L.strsim_pairs_device_small.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, vp, u64]
    rc = L.strsim_pairs_device_small(ctx._h, 10, t[0].data_ptr(), t[1].data_ptr(), len(A), t[2].data_ptr(), t[3].data_ptr(), len(A),
                                     out.data_ptr(), len(A))
    assert rc == 0
    ctx.synchronize()
    assert ctx.last_long_rows == 0
    same_bits(out.cpu().numpy(), exp_s)
    # two calls back to back on one context, results read after both
    o1 = ctx.pairs_device("partial_ratio", *t)
    s2, sp2 = ctx.partial_alignment_device(*t)
    o3 = ctx.pairs_device("indel", *t)
    ctx.synchronize()
    same_bits(o1.cpu().numpy(), exp_s)
    same_bits(s2.cpu().numpy(), exp_s)
    same_spans(sp2.cpu().numpy().view(np.uint32), exp_sp)
    import indel_ref
    same_bits(o3.cpu().numpy(), [indel_ref.score(a, b) for a, b in zip(A, B)])


def test_alignment_score_equals_pairwise_on_the_mixed_frame(S, ctx):
    A, B = gen.pairs(1008, 60_000, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(1009, 20_000, gen.MIXED, 0, 60)
    A3, B3 = gen.pairs(1010, 2_000, gen.ASCII_LOWER, 20, 128, max_bytes=128)
    A, B = A + A2 + A3, B + B2 + B3
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    s1 = ctx.pairs_host("partial_ratio", ao, av, bo, bv)
    s2, sp = ctx.partial_alignment_host(ao, av, bo, bv)
    same_bits(s2, s1)
    la = np.array([len(a) for a in A]); lb = np.array([len(b) for b in B])
    both = (la > 0) & (lb > 0)
    assert ((sp[:, 1] - sp[:, 0])[both] >= 1).all() and (sp[:, 1] <= la).all() and (sp[:, 3] <= lb).all()
    assert ((sp[:, 1] - sp[:, 0] == la) | (sp[:, 3] - sp[:, 2] == lb))[both].all()
