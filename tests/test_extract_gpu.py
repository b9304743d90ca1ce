"""Extract on the MI355X (strsim_extract_*) against the contract stated independently: the score of every pair from indel_ref /
token_ref, then best_match_ref's NumPy top-k (tests/extract_ref.py) -- descending score, ties to the lower candidate index, the
cutoff applied.  Every comparison is exact: indices equal, scores bit for bit."""
import functools
import math
import random

import numpy as np
import pytest

import extract_ref as R
import gen
import indel_ref
import token_ref

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")
SCORERS = R.SCORERS
MEASURE = {"ratio": "indel", "token_sort_ratio": "token_sort_ratio"}
INF = float("inf")


def E(d, s):
    return indel_ref.normalise(d, s, 0)


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def _run(ctx, scorer, Q, Cs, k, cut=None):
    qo, qv = S.pack_strings(Q)
    co, cv = S.pack_strings(Cs)
    idx, score = ctx.extract(MEASURE[scorer], qo, qv, co, cv, k, cut)
    empty = idx == 0xFFFFFFFF
    assert np.array_equal(empty, np.isnan(score))
    return np.where(empty, -1, idx.astype(np.int64)), score


def _same(got, exp, rows=None):
    gi, gs = got
    ei, es = exp
    if rows is not None:
        gi, gs = gi[rows], gs[rows]
    assert gi.shape == ei.shape
    bad = np.argwhere((gi != ei) | (np.ascontiguousarray(gs).view(np.uint64) != np.ascontiguousarray(es).view(np.uint64)))
    assert bad.size == 0, "row %d differs: got %s / %s, expected %s / %s" % (
        bad[0][0], gi[bad[0][0]].tolist(), gs[bad[0][0]].tolist(), ei[bad[0][0]].tolist(), es[bad[0][0]].tolist())


def _check(ctx, scorer, Q, Cs, k, cut=None, scores=None):
    got = _run(ctx, scorer, Q, Cs, k, cut)
    _same(got, R.topk(R.score_matrix(scorer, Q, Cs) if scores is None else scores, k, cut))
    return got


def _strings(seed, n, alphabet=gen.ASCII_LOWER, lo=0, hi=32):
    A, B = gen.pairs(seed, (n + 1) // 2, alphabet, lo, hi)
    return (A + B)[:n]


def _tokens(seed, n):
    """token_ref's frame: 1-4 tokens of 1-6 letters, half the rows a shuffled and edited copy of another"""
    A, B = token_ref.gen_frame(seed, (n + 1) // 2)
    return (A + B)[:n]


def _frame(scorer, seed, n, **kw):
    """strings that exercise the scorer: multi-token rows for token_sort_ratio"""
    return _tokens(seed, n) if scorer == "token_sort_ratio" and not kw else _strings(seed, n, **kw)


def _near_duplicates(seed, cands, n, alphabet=gen.ASCII_LOWER):
    """each query a random candidate with 0..3 random edits (insert, delete, substitute, adjacent swap)"""
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


@functools.lru_cache(maxsize=None)
def _random_ascii(scorer):
    Q = _strings(11, 300, lo=0, hi=12)
    Cs = _strings(12, 500, lo=0, hi=12)
    if scorer == "token_sort_ratio":  # the same strings with some letters turned into spaces: tokens to sort
        Q = [s.replace("e", " ").replace("t", " ") for s in Q]
        Cs = [s.replace("e", " ").replace("t", " ") for s in Cs]
    M = R.score_matrix(scorer, Q, Cs)
    M.setflags(write=False)
    return Q, Cs, M


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("cut", [None, 0.0, 0.5, 0.8, 1.0, 1.5])
def test_extract_gpu_random_ascii(ctx, scorer, k, cut):
    Q, Cs, M = _random_ascii(scorer)
    gi, gs = _check(ctx, scorer, Q, Cs, k, cut, M)
    if cut == 1.5:
        assert (gi == -1).all()
    if cut in (None, 0.0):
        assert (gi >= 0).all()


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_edge_lengths(ctx, scorer):
    # 0, 1, 31, 32 take the lane path, 33 the fallback; near copies across the lengths
    rng = random.Random(5)
    base = "".join(rng.choice("abcd") for _ in range(33))
    Q = [base[:n] for n in (0, 1, 31, 32, 33)] + [base[1:32], base[:30] + "zz", "", "a"]
    Cs = [base[:n] for n in (0, 1, 2, 30, 31, 32, 33)] + [base[2:33], base[:31] + "x", "b", ""]
    M = R.score_matrix(scorer, Q, Cs)
    for k in (1, 3, 16):
        for cut in (None, 0.0, 5e-324, 0.5, 0.9, 1.0):
            _check(ctx, scorer, Q, Cs, k, cut, M)
    # empty against empty is 1.0; empty against a non-empty candidate is reported at 0.0 with no cutoff ...
    gi, gs = _run(ctx, scorer, [""], ["abc", "", "x"], 3)
    assert gi.tolist() == [[1, 0, 2]] and gs.tolist() == [[1.0, 0.0, 0.0]]
    gi, gs = _run(ctx, scorer, [""], ["abc", "x"], 3, 0.0)
    assert gi.tolist() == [[0, 1, -1]] and gs[0, :2].tolist() == [0.0, 0.0]
    # ... and dropped at any cutoff above 0
    for cut in (5e-324, 0.01, 1.0):
        gi, gs = _run(ctx, scorer, [""], ["abc", "", "x"], 3, cut)
        assert gi.tolist() == [[1, -1, -1]] and gs[0, 0] == 1.0


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_heavy_ties(ctx, scorer):
    # duplicate candidates and a two-letter alphabet: many equal scores, decided by the index
    Q = _strings(21, 400, alphabet="ab", lo=1, hi=6)
    base = _strings(22, 60, alphabet="ab", lo=1, hi=6)
    Cs = base + base[::-1] + base
    M = R.score_matrix(scorer, Q, Cs)
    for k in (1, 3, 16):
        for cut in (0.5, None):
            _check(ctx, scorer, Q, Cs, k, cut, M)
    # the cross-length tie: "ba" (d 2, s 4) and "abxxxx" (d 4, s 8) both score 0.5 against "ab"; the lower index wins
    # whichever length the sweep visits first
    for Cs2 in (["ba", "abxxxx"], ["abxxxx", "ba"], ["zz", "abxxxx", "ba", "ba", "abxxxx"]):
        for k in (1, 4):
            gi, gs = _check(ctx, scorer, ["ab"] * 70 + ["abc"], Cs2, k)
            assert gs[0, 0] == 0.5 and gi[0, 0] == min(j for j, c in enumerate(Cs2) if c != "zz")


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_cutoff_at_an_attainable_score_and_its_neighbours(ctx, scorer):
    Q, Cs, M = _random_ascii(scorer)
    for v in (E(2, 6), E(3, 7), 0.5):
        assert (M == v).any()
        cuts = (math.nextafter(v, -INF), v, math.nextafter(v, INF))
        kept = []
        for cut in cuts:
            gi, gs = _check(ctx, scorer, Q, Cs, 16, cut, M)
            kept.append(int((gi >= 0).sum()))
            assert (gs[gi >= 0] >= cut).all()
        assert kept[0] == kept[1] > kept[2]  # the cutoff is inclusive: only the next double above v drops the pairs at v


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_empty_candidates_and_k_above_rows(ctx, scorer):
    Q = ["abc", "", "xyz"]
    gi, gs = _run(ctx, scorer, Q, [], 3)
    assert (gi == -1).all() and np.isnan(gs).all()
    _check(ctx, scorer, Q, ["ab", "abcd"], 16)
    _check(ctx, scorer, Q, ["ab", "abcd"], 16, 0.6)
    gi, gs = _run(ctx, scorer, [], ["a"], 4)
    assert gi.shape == (0, 4)


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_mixed_case_five_and_seven_planes(ctx, scorer):
    # a wave of lowercase queries runs five planes against lowercase candidates and seven against mixed-case ones
    Q = _strings(31, 256, lo=1, hi=16) + _strings(32, 128, alphabet="abcXYZ09 -", lo=1, hi=16)
    Cs = _strings(33, 300, lo=1, hi=16) + _strings(34, 100, alphabet="aBcXyZ09_ ", lo=1, hi=16) + ["HELLO", "hello", "Hello"]
    M = R.score_matrix(scorer, Q, Cs)
    for k in (1, 16):
        _check(ctx, scorer, Q, Cs, k, None, M)
        _check(ctx, scorer, Q, Cs, k, 0.6, M)


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("side", ["queries", "candidates", "both"])
def test_extract_gpu_slow_strings(ctx, scorer, side):
    # non-ASCII and > 32-byte strings go through strsim_pairs_device(STRSIM_INDEL), scored once per pair
    fast_q = _frame(scorer, 41, 150)
    fast_c = _frame(scorer, 42, 120)
    slow_q = ["héllo wörld", "日本語テキスト", "x" * 40, "kitten" * 6, "ab " * 12, "ñ"]
    slow_c = ["hello world", "wörld héllo", "y" * 33, "kitten" * 6 + "s", "日本語", "ab " * 12, "n"]
    Q = fast_q + (slow_q if side in ("queries", "both") else [])
    Cs = fast_c + (slow_c if side in ("candidates", "both") else []) + ["world hello"]
    rng = random.Random(43)
    rng.shuffle(Q)
    rng.shuffle(Cs)
    M = R.score_matrix(scorer, Q, Cs)
    for k in (1, 3, 16):
        for cut in (0.7, None):
            _check(ctx, scorer, Q, Cs, k, cut, M)


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("side", ["queries", "candidates", "both"])
@pytest.mark.parametrize("k", [1, 3])
def test_extract_gpu_more_slow_strings_than_one_batch(ctx, scorer, side, k):
    # 37 slow queries and 21 slow candidates (gen.batch_boundary_frame): the fallback folds three batches of slow queries and
    # two of slow candidates into its list
    Q, Cs = gen.batch_boundary_frame(191, side)
    M = R.score_matrix(scorer, Q, Cs)
    for cut in (0.5, None):
        _check(ctx, scorer, Q, Cs, k, cut, M)


def test_extract_gpu_token_sort_normalises_on_the_device(ctx):
    # permuted tokens, runs of whitespace, multi-byte whitespace code points (U+3000), tokenless strings.  Raw strings longer than
    # 32 bytes whose normalised form is a lane-path string (runs of spaces), raw strings of at most 32 bytes that k_match_pack
    # would refuse (non-ASCII whitespace) but whose normalised form is ASCII, and strings that stay long or non-ASCII.
    Q = ["new york mets", "mets  york   new", "  york\tnew\nmets ", "york　new mets", "a b", "", "   ", "　　",
         "b    a          c          d      e", "the quick brown fox jumps over the lazy dog", "dog lazy the over jumps fox brown quick the",
         "z" * 20 + "          " + "y" * 12, "é b a", "fox"] + _tokens(55, 200)
    Cs = ["mets new york", "york mets", "new  york", "a b", "b a", "", " \t ", "a b c d e", "e d c b a" + " " * 30,
          "quick the brown fox the lazy dog jumps over", "y" * 12 + " " + "z" * 20, "a b é", "fox  "] + _tokens(56, 300)
    rng = random.Random(57)
    rng.shuffle(Q)
    rng.shuffle(Cs)
    M = R.score_matrix("token_sort_ratio", Q, Cs)
    for k in (1, 3, 16):
        for cut in (None, 0.75, 1.0):
            got = _check(ctx, "token_sort_ratio", Q, Cs, k, cut, M)
            # the same search over the columns normalised by the GPU's own transform
            _same(_run(ctx, "ratio", S.token_sort(Q, ctx=ctx), S.token_sort(Cs, ctx=ctx), k, cut), got)
    i = Q.index("mets  york   new")
    gi, gs = _run(ctx, "token_sort_ratio", Q, Cs, 1)
    assert Cs[gi[i, 0]] == "mets new york" and gs[i, 0] == 1.0


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_near_duplicates_dynamic_bound(ctx, scorer):
    # most queries have a candidate within 3 edits, so the bound of a full list cuts the sweep short; sampled rows against the model
    Cs = _strings(51, 1000, lo=4, hi=24)
    if scorer == "token_sort_ratio":
        Cs = [s[:len(s) // 2] + " " + s[len(s) // 2:] for s in Cs]
    Q = _near_duplicates(52, Cs, 3000)
    rows = np.random.default_rng(53).choice(len(Q), 48, replace=False)
    M = R.score_matrix(scorer, [Q[i] for i in rows], Cs)
    for k in (1, 4):
        for cut in (None, 0.8):
            got = _run(ctx, scorer, Q, Cs, k, cut)
            _same(got, R.topk(M, k, cut), rows)
            if cut is None and k == 1:  # (each edit costs at most 2 in d, and the strings have at least 4 characters)
                assert (got[1][:, 0] >= 0.5).mean() > 0.9


@functools.lru_cache(maxsize=None)
def _split_frame(scorer):
    Q = _strings(61, 2000, lo=0, hi=12)
    Cs = _strings(62, 200_000, lo=0, hi=12)
    if scorer == "token_sort_ratio":
        Q = [s.replace("e", " ") for s in Q]
        Cs = [s.replace("e", " ") for s in Cs]
    rows = np.random.default_rng(63).choice(len(Q), 4, replace=False)
    M = R.score_matrix(scorer, [Q[i] for i in rows], Cs)
    return Q, Cs, rows, M


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_split_frame_few_queries(ctx, scorer):
    # 2 k queries x 200 k candidates: few query waves, so the candidates are split over grid.y and the lists merged
    Q, Cs, rows, M = _split_frame(scorer)
    _same(_run(ctx, scorer, Q, Cs, 3, None), R.topk(M, 3, None), rows)
    _same(_run(ctx, scorer, Q, Cs, 1, 0.8), R.topk(M, 1, 0.8), rows)


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_split_frame_square(ctx, scorer):
    Q = _strings(71, 20_000, lo=0, hi=14)
    Cs = _near_duplicates(72, Q[:5000], 20_000)
    if scorer == "token_sort_ratio":
        Q = [s.replace("e", " ") for s in Q]
        Cs = [s.replace("e", " ") for s in Cs]
    rows = np.random.default_rng(73).choice(len(Q), 12, replace=False)
    M = R.score_matrix(scorer, [Q[i] for i in rows], Cs)
    _same(_run(ctx, scorer, Q, Cs, 16, None), R.topk(M, 16, None), rows)
    _same(_run(ctx, scorer, Q, Cs, 1, 0.9), R.topk(M, 1, 0.9), rows)


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_permuted_candidates_map_back(ctx, scorer):
    # the same search over a permuted candidate column: the same scores row by row, each answer maps back (through the
    # permutation) to a candidate with that score, and the lists are exactly the reference's for the permuted order
    Q = _frame(scorer, 81, 200)
    Cs = _frame(scorer, 82, 300) + ["Zürich", "z" * 35]
    perm = np.random.default_rng(83).permutation(len(Cs))
    M = R.score_matrix(scorer, Q, Cs)
    a_i, a_s = _run(ctx, scorer, Q, Cs, 16, 0.6)
    b_i, b_s = _run(ctx, scorer, Q, [Cs[j] for j in perm], 16, 0.6)
    assert np.array_equal(a_s.view(np.uint64), b_s.view(np.uint64))
    I, J = np.nonzero(b_i >= 0)
    assert np.array_equal(M[I, perm[b_i[I, J]]], b_s[I, J])
    _same((b_i, b_s), R.topk(M[:, perm], 16, 0.6))


def test_extract_gpu_repeatable(ctx):
    Q = _strings(91, 5000, alphabet="abc ", lo=0, hi=12)
    Cs = _strings(92, 3000, alphabet="abc ", lo=0, hi=12)
    for scorer in SCORERS:
        a = _run(ctx, scorer, Q, Cs, 16)
        b = _run(ctx, scorer, Q, Cs, 16)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_gpu_agrees_with_pairwise_calls(ctx, scorer):
    # every reported (i, j, score) is what strsim_pairs_device(scorer) returns for that pair, bit for bit
    Q = _frame(scorer, 101, 200) + ["héllo wörld", "q" * 40, "a  b"]
    Cs = _frame(scorer, 102, 300) + ["wörld hello", "q" * 39, "b a"]
    gi, gs = _run(ctx, scorer, Q, Cs, 16, 0.3)
    I, J = np.nonzero(gi >= 0)
    jj = gi[I, J]
    qo, qv = S.pack_strings([Q[i] for i in I])
    co, cv = S.pack_strings([Cs[j] for j in jj])
    v = ctx.pairs_host(MEASURE[scorer], qo, qv, co, cv)
    assert np.array_equal(v.view(np.uint64), np.ascontiguousarray(gs[I, J]).view(np.uint64))


def test_extract_gpu_device_resident_inputs(ctx):
    # torch tensors on the device in, torch tensors out (strsim_extract_device), complete after ctx.synchronize()
    torch = pytest.importorskip("torch")
    Q, Cs, M = _random_ascii("ratio")
    dev = torch.device("cuda", 0)
    cols = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.uint8)).to(dev)
            for x in (*S.pack_strings(Q), *S.pack_strings(Cs))]
    torch.cuda.synchronize()
    idx, score = ctx.extract("indel", *cols, k=3, score_cutoff=0.5)
    ctx.synchronize()
    gi = idx.cpu().numpy().astype(np.int64)  # (int32: an empty slot reads -1)
    _same((gi, score.cpu().numpy()), R.topk(M, 3, 0.5))


def test_extract_gpu_python_wrapper_nulls(ctx):
    Q = ["kitten", None, "abc", "zzzz"]
    Cs = [None, "sitting", "abd", None, "kitten"]
    idx, score = S.extract("ratio", Q, Cs, k=2, score_cutoff=0.5, ctx=ctx)
    assert idx.tolist() == [[4, 1], [-1, -1], [2, -1], [-1, -1]]
    assert score[0].tolist() == [1.0, E(5, 13)] and score[2, 0] == E(2, 6) and np.isnan(score[1]).all() and np.isnan(score[3]).all()
    assert np.isnan(score[2, 1])
    idx, score = S.extract("token_sort_ratio", ["b a"], [None, "ab", "a  b"], ctx=ctx)
    assert idx.tolist() == [[2]] and score.tolist() == [[1.0]]
    idx2, score2 = S.extract("indel", Q, Cs, k=2, score_cutoff=0.5, ctx=ctx)
    assert idx2.tolist() == [[4, 1], [-1, -1], [2, -1], [-1, -1]]
