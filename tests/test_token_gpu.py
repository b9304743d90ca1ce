"""token_sort_ratio / token_set_ratio (measures 14 and 16) and the token_sort transform on the GPU, bit for bit (f64) and byte for
byte (the transform) against tests/token_ref.py: known answers, every tier boundary of the transform, every whitespace code point,
tokenless rows, duplicates, prefixes, NUL, non-ASCII tokens, 1 000 tokens, 100 kB, literals, zero rows, nulls, device-resident
calls, interleaved calls on one context, what a frame leaves for the one-string-per-wave tier, random frames and a 10 M-row frame."""
import random

import numpy as np
import pytest

import indel_ref
import token_ref as R

pytestmark = pytest.mark.gpu

LANE_BYTES, LANE_TOKENS = 64, 16  # TOKEN_LANE_MAX_BYTES, TOKEN_LANE_MAX_TOKENS of strsim_token.h
LDS_TOKENS = 1024                 # TOKEN_WAVE_LDS_TOKENS


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
    return indel_ref.CRef()


def same_bits(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, [(int(i), float(got[i]), float(exp[i])) for i in bad[:8]]


def gpu(S, ctx, measure, A, B):
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    return ctx.pairs_host(measure, ao, av, bo, bv)


def model(measure, A, B, lcs_fn=R.lcs):
    A, B = R.broadcast(list(A), list(B))
    f = R.token_sort_ratio if measure == "token_sort_ratio" else R.set_rule
    return np.array([f(a, b, lcs_fn) for a, b in zip(A, B)], dtype=np.float64)


def lane_string(s):
    """What the one-string-per-lane tier takes."""
    return s.isascii() and len(s) <= LANE_BYTES and len(s.split()) <= LANE_TOKENS


def check(S, ctx, A, B, lcs_fn=R.lcs, transform=True):
    """Both measures and (transform) the transform of both columns against the model; checks the wave-tier counter too."""
    for m in ("token_sort_ratio", "token_set_ratio"):
        same_bits(gpu(S, ctx, m, A, B), model(m, A, B, lcs_fn))
        ctx.synchronize()
        if m == "token_sort_ratio":
            want = sum(not lane_string(s) for s in A) + sum(not lane_string(s) for s in B)
        else:
            X, Y = R.broadcast(list(A), list(B))
            want = sum(not (lane_string(a) and lane_string(b)) for a, b in zip(X, Y))
        assert ctx.last_token_wave_rows == want, (m, ctx.last_token_wave_rows, want)
    if transform:
        for col in (A, B):
            assert S.token_sort(col, ctx=ctx) == [R.token_sort(s) for s in col]


def test_known_answers(S, ctx):
    A = ["fuzzy wuzzy was a bear", "fuzzy was a bear", "smith john", "b a", "a a", " \t", "  ", "ab", "x ab", "x y z a"]
    B = ["wuzzy fuzzy was a bear", "fuzzy fuzzy was a bear", "john  smith", "a c", "a", "", "a", "cd", "ac x", "b z y x"]
    sort_exp = [1.0, None, 1.0, 1.0 - 2.0 / 6.0, 0.5, 1.0, 0.0, 0.0, None, None]
    set_exp = [None, 1.0, 1.0, None, 1.0, 0.0, 0.0, 0.0, 0.75, 1.0 - 2.0 / 14.0]  # (derivations: tests/test_token_cpu.py)
    got_sort, got_set = S.token_sort_ratio(A, B, ctx=ctx), S.token_set_ratio(A, B, ctx=ctx)
    for i in range(len(A)):
        if sort_exp[i] is not None:
            assert got_sort[i] == sort_exp[i], (i, got_sort[i])
        if set_exp[i] is not None:
            assert got_set[i] == set_exp[i], (i, got_set[i])
    same_bits(got_sort, model("token_sort_ratio", A, B))
    same_bits(got_set, model("token_set_ratio", A, B))
    same_bits(S.similarity("token_sort_ratio", B, A, ctx=ctx), model("token_sort_ratio", B, A))
    same_bits(S.similarity("token_set_ratio", B, A, ctx=ctx), model("token_set_ratio", B, A))
    assert S.token_sort(["smith john", "john  smith", "", None, " ", "ab a abc \0"], ctx=ctx) == ["john smith", "john smith", "", None, "",
                                                                                                   "\0 a ab abc"]


def test_tier_boundaries(S, ctx, cref):
    rng = random.Random(5)

    def words(n_tokens, total):
        """n_tokens tokens over 'abc' in exactly `total` bytes (single spaces)."""
        free = total - (n_tokens - 1)
        lens = [1] * n_tokens
        for _ in range(free - n_tokens):
            lens[rng.randrange(n_tokens)] += 1
        return " ".join("".join(rng.choice("abc") for _ in range(k)) for k in lens)

    A, B = [], []
    for total in (63, 64, 65, 66):            # the last length inside the lane tier and the first outside
        for nt in (1, 5, 16):
            A.append(words(nt, total))
            B.append(words(nt, total - 1))
    for nt in (15, 16, 17, 18):               # the last token count inside and the first outside
        A.append(words(nt, 2 * nt + 3))
        B.append(words(16, 40))
    A += [" ".join("a" for _ in range(17)), " ".join("a" for _ in range(16)), "a " * 32, " a" * 32, " " * 64, " " * 65]
    B += [" ".join("a" for _ in range(16)), " ".join("b" for _ in range(17)), "a", "b a", "", " "]
    A += ["abc déf", "abc def", "é" * 32, "x" * 62 + "é"]   # ASCII against not ASCII, bytes against characters
    B += ["abc def", "abc déf", "e" * 64, "x" * 64]
    # the descriptors of the wave tier: in LDS up to 1 024 possible tokens (2 048 bytes; set form: both strings together)
    for total in (2047, 2048, 2049, 2050):
        A.append(words(total // 2, total))
        B.append(words(40, 200))
    for la, lb in ((1023, 1023), (1024, 1024), (1025, 1023), (1025, 1025)):
        A.append(words(la // 2, la))
        B.append(words(lb // 2, lb))
    assert any(lane_string(s) for s in A) and any(not lane_string(s) for s in A)
    check(S, ctx, A, B, cref.lcs)
    check(S, ctx, B, A, cref.lcs, transform=False)


def test_whitespace_duplicates_prefixes_nul_and_non_ascii(S, ctx):
    ws = [chr(c) for c in R.WHITESPACE]
    A = ["  lead", "trail  ", " both  ", "a   b\t\tc\n", "", " ", "\t\n\x0b\x0c\r\x1c\x1d\x1e\x1f \x85\xa0", "".join(ws), "a a a", "b a b a",
         "ab a abc abcd", "a\0b \0 \0\0", "\0", "жук бук", "漢字 漢 字", "naïve café \U0001F600",
         "\u200bzero \u200b width", "\u1681 \u2027 \u00c2 \u00c2\u0085x"]
    B = ["lead", "trail", "both", "c b a", " ", "", "x", "", "a", "a b",
         "abcd abc a ab", "\0\0 \0 a\0b", "\0 \0", "бук жук", "字 漢字", "café \U0001F600 naive",
         "zero width", "\u00c2 x \u1681"]
    for c in ws:  # every whitespace code point as a separator, leading, trailing and doubled
        A += ["b" + c + "a", c + "a" + c + c + "b" + c, "é" + c + "a"]
        B += ["a b", "b" + c + "a", "a" + c + "é"]
    check(S, ctx, A, B)
    check(S, ctx, B, A, transform=False)
    rng = random.Random(17)
    alphabet = ws + ["\0", "a", "b", "c", "ab", "ж", "я", "漢", "字", "\U0001F600", "\u200b", "\u1681", "\u2027", "\u00c2"]
    A = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 14))) for _ in range(4000)]
    B = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 14))) for _ in range(4000)]
    check(S, ctx, A, B)


def test_thousand_tokens_and_100_kb(S, ctx, cref):
    rng = random.Random(23)
    letters = "abcdefghijklmnopqrstuvwxyz"
    thousand = " ".join(rng.choice(letters) for _ in range(1000))
    toks = ["".join(rng.choice(letters) for _ in range(rng.randint(1, 12))) for _ in range(16000)]
    big = "  ".join(toks)[:100_000].rstrip()
    assert len(big) >= 99_000 and len(big.split()) > 10_000
    partner = " ".join(rng.sample(big.split(), 150) + ["zzzz", "q"])
    one_token = "x" * 100_000
    A = [thousand, big, one_token, "short row", big]
    B = [" ".join(reversed(thousand.split())), partner, "x" * 500 + " y", thousand, "a b"]
    assert S.token_sort(A, ctx=ctx) == [R.token_sort(s) for s in A]
    for m in ("token_sort_ratio", "token_set_ratio"):
        same_bits(gpu(S, ctx, m, A, B), model(m, A, B, cref.lcs))
        same_bits(gpu(S, ctx, m, B, A), model(m, B, A, cref.lcs))


def test_literals_and_zero_rows(S, ctx, cref):
    A, B = R.gen_frame(31, 5000)
    A += ["", "  ", "café naïve", "x" * 70, " ".join("t%d" % i for i in range(20))]
    for lit in (["ab cd"], [""], [" "], ["déjà vu café"], [" ".join("t%d" % i for i in range(20, 0, -1))], [A[3]]):
        for m in ("token_sort_ratio", "token_set_ratio"):
            same_bits(gpu(S, ctx, m, A, lit), model(m, A, lit, cref.lcs))
            same_bits(gpu(S, ctx, m, lit, A), model(m, lit, A, cref.lcs))
            same_bits(gpu(S, ctx, m, lit, lit), model(m, lit, lit, cref.lcs))
    for m in ("token_sort_ratio", "token_set_ratio"):
        assert gpu(S, ctx, m, [], []).size == 0
        assert S.similarity(m, [], [], ctx=ctx).size == 0
        with pytest.raises(S.ShapeMismatch):
            gpu(S, ctx, m, ["a", "b"], ["a", "b", "c"])
    assert S.token_sort([], ctx=ctx) == []
    off, val = ctx.token_sort_host(np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint8))
    assert off.tolist() == [0] and val.size == 0


def test_nulls_through_similarity(S, ctx):
    A = ["b a", None, "c", None, "x y"]
    B = ["a b", "a", None, None, "y"]
    for m, exp in (("token_sort_ratio", [1.0, None, None, None, R.token_sort_ratio("x y", "y")]),
                   ("token_set_ratio", [1.0, None, None, None, 1.0])):
        got = S.similarity(m, A, B, ctx=ctx)
        for g, e in zip(got, exp):
            assert (np.isnan(g) and e is None) or g == e
        got = S.similarity(m, A, None, ctx=ctx)
        assert np.isnan(got).all()
        got = S.similarity(m, "a b", B, ctx=ctx)
        assert np.isnan(got[2]) and np.isnan(got[3]) and got[0] == 1.0


def test_host_paths_agree(S, cref, monkeypatch):
    """strsim_pairs_host computes small calls in place on pinned memory and stages large ones: both against the model."""
    A, B = R.gen_frame(41, 3000)
    A += ["漢字 漢", "w" * 90 + " v"]
    B += ["漢 字", "v " + "w" * 90]
    for direct in ("0", None):
        if direct is not None:
            monkeypatch.setenv("STRSIM_HOST_DIRECT_ROWS", direct)
        else:
            monkeypatch.delenv("STRSIM_HOST_DIRECT_ROWS", raising=False)
        with S.Context(0) as c:
            for m in ("token_sort_ratio", "token_set_ratio"):
                same_bits(gpu(S, c, m, A, B), model(m, A, B, cref.lcs))
                same_bits(gpu(S, c, m, A[:1], B), model(m, A[:1], B, cref.lcs))


def test_device_calls_and_what_a_frame_leaves_behind(S):
    import torch
    A, B = R.gen_frame(51, 60_000)
    assert all(lane_string(s) for s in A + B)
    A2 = ["café au lait", "y" * 65, " ".join("t" for _ in range(17)), "plain"]
    B2 = ["lait café", "y" * 64, "t", "é"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
    exp = {m: R.frame_sort_ratio(A, B) if m == "token_sort_ratio" else R.frame_set_ratio(A, B) for m in S.TOKEN_MEASURES}
    exp2 = {m: model(m, A2, B2) for m in S.TOKEN_MEASURES}
    for one_launch in (False, True):
        with S.Context(0, one_launch=one_launch) as c:
            ao, av = (dev(x) for x in S.pack_strings(A))
            bo, bv = (dev(x) for x in S.pack_strings(B))
            ao2, av2 = (dev(x) for x in S.pack_strings(A + A2))
            bo2, bv2 = (dev(x) for x in S.pack_strings(B + B2))
            for m in S.TOKEN_MEASURES:
                out = c.pairs_device(m, ao, av, bo, bv)
                torch.cuda.synchronize()
                c.synchronize()
                same_bits(out.cpu().numpy(), exp[m])
                # a frame where no row reaches a one-string-per-wave tier says so, in the transform and in the Indel pass behind it
                assert c.last_token_wave_rows == 0 and c.last_late_rows == 0 and c.last_long_rows == 0
                if m == "token_sort_ratio":
                    assert c.last_wave_rows == 0
                out = c.pairs_device(m, ao2, av2, bo2, bv2)
                c.synchronize()
                same_bits(out.cpu().numpy(), np.concatenate([exp[m], exp2[m]]))
                assert c.last_token_wave_rows == (3 + 2 if m == "token_sort_ratio" else 4)
            # the transform, device-resident; then Indel over the normalised columns is token_sort_ratio
            na = c.token_sort_device(ao2, av2)
            nb = c.token_sort_device(bo2, bv2)
            c.synchronize()
            assert c.last_token_wave_rows == 2
            off = na[0].cpu().numpy().view(np.uint32)
            raw = na[1].cpu().numpy().tobytes()
            assert [raw[off[i]:off[i + 1]].decode() for i in range(len(A) + len(A2))] == [R.token_sort(s) for s in A + A2]
            out = c.pairs_device("indel", na[0], na[1], nb[0], nb[1])
            c.synchronize()
            same_bits(out.cpu().numpy(), np.concatenate([exp["token_sort_ratio"], exp2["token_sort_ratio"]]))
            # a capacity below the column's bytes is refused
            with pytest.raises(S.StrsimError, match="out_capacity"):
                c.token_sort_device(ao2, av2, out_values=torch.empty(av2.numel() - 1, dtype=torch.uint8, device="cuda:0"))


def test_interleaved_calls_on_one_context(S, cref):
    """token_set_ratio, indel, token_sort_ratio and partial_ratio interleaved: scratch and the work lists are not shared wrongly."""
    import partial_ref
    A, B = R.gen_frame(61, 20_000)
    A += ["café au lait", "z" * 80 + " y", ""]
    B += ["lait café", "y " + "z" * 80, "q"]
    exp = {"token_set_ratio": model("token_set_ratio", A, B, cref.lcs), "token_sort_ratio": model("token_sort_ratio", A, B, cref.lcs),
           "indel": np.array([R.indel(a, b, cref.lcs) for a, b in zip(A, B)])}
    small_a, small_b = A[-40:], B[-40:]
    exp_partial = np.array([partial_ref.partial(a, b)[0] for a, b in zip(small_a, small_b)])
    import torch
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
    with S.Context(0) as c:
        ao, av = (dev(x) for x in S.pack_strings(A))
        bo, bv = (dev(x) for x in S.pack_strings(B))
        so, sv = (dev(x) for x in S.pack_strings(small_a))
        to, tv = (dev(x) for x in S.pack_strings(small_b))
        outs = []
        for _ in range(3):  # enqueued back to back, read afterwards
            for m in ("token_set_ratio", "indel", "token_sort_ratio"):
                outs.append((m, c.pairs_device(m, ao, av, bo, bv)))
            outs.append(("partial", c.pairs_device("partial_ratio", so, sv, to, tv)))
            outs.append(("token_set_ratio", c.pairs_device("token_set_ratio", bo, bv, ao, av)))
        c.synchronize()
        for m, out in outs:
            same_bits(out.cpu().numpy(), exp_partial if m == "partial" else exp[m])


def test_random_frames(S, ctx):
    for seed, n in ((71, 200_000), (72, 50_000)):
        A, B = R.gen_frame(seed, n)
        for m, exp in (("token_sort_ratio", R.frame_sort_ratio(A, B)), ("token_set_ratio", R.frame_set_ratio(A, B))):
            # (on the model's output) a frame of mostly 0.0 / 1.0 would prove little
            assert float(((exp == 0.0) | (exp == 1.0)).mean()) <= 0.30
            same_bits(gpu(S, ctx, m, A, B), exp)


def test_large_frame(S):
    """10.4 M rows (a generated block tiled on the device): windows against the model, and every row by the cross-check
    token_sort_ratio(a, b) == indel(token_sort(a), token_sort(b)), all on the GPU."""
    import torch
    block, tiles = 104_000, 100
    A, B = R.gen_frame(81, block)

    def tiled(strings):
        off, val = S.pack_strings(strings)
        o = torch.from_numpy(off.astype(np.int64)).to("cuda:0")
        v = torch.from_numpy(val).to("cuda:0")
        total = int(off[-1])
        offs = (o[:-1].unsqueeze(0) + torch.arange(tiles, device="cuda:0", dtype=torch.int64).unsqueeze(1) * total).reshape(-1)
        offs = torch.cat([offs, torch.tensor([tiles * total], device="cuda:0", dtype=torch.int64)])
        return offs.to(torch.int32).contiguous(), v.repeat(tiles).contiguous()

    n = block * tiles
    assert n >= 10_000_000
    with S.Context(0) as c:
        ao, av = tiled(A)
        bo, bv = tiled(B)
        sort = c.pairs_device("token_sort_ratio", ao, av, bo, bv)
        c.synchronize()
        assert c.last_token_wave_rows == 0
        sset = c.pairs_device("token_set_ratio", ao, av, bo, bv)
        na = c.token_sort_device(ao, av)
        nb = c.token_sort_device(bo, bv)
        cross = c.pairs_device("indel", na[0], na[1], nb[0], nb[1])
        c.synchronize()
        assert torch.equal(sort.view(torch.int64), cross.view(torch.int64))
        exp_sort, exp_set = R.frame_sort_ratio(A[:4000], B[:4000]), R.frame_set_ratio(A[:4000], B[:4000])
        for t in (0, 1, 57, tiles - 1):  # windows: the head of a tile, and the seam between the last two
            lo = t * block
            same_bits(sort[lo:lo + 4000].cpu().numpy(), exp_sort)
            same_bits(sset[lo:lo + 4000].cpu().numpy(), exp_set)
        tail_sort, tail_set = R.frame_sort_ratio(A[-3000:], B[-3000:]), R.frame_set_ratio(A[-3000:], B[-3000:])
        same_bits(sort[n - 3000:].cpu().numpy(), tail_sort)
        same_bits(sset[n - 3000:].cpu().numpy(), tail_set)
        # every tile equals the first one
        assert torch.equal(sort.view(tiles, block).view(torch.int64), sort[:block].view(torch.int64).unsqueeze(0).expand(tiles, block))
        assert torch.equal(sset.view(tiles, block).view(torch.int64), sset[:block].view(torch.int64).unsqueeze(0).expand(tiles, block))
