"""Best match on the MI355X (strsim_best_match_*, ABI 1.7) against the contract stated independently: the CPU oracle's score of
every pair, then a NumPy top-k (tests/best_match_ref.py).  Indices exactly, scores bit for bit."""
import random

import numpy as np
import pytest

import best_match_ref as R
import gen

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")
MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def _run(ctx, measure, Q, Cs, k, min_score=None):
    qo, qv = S.pack_strings(Q)
    co, cv = S.pack_strings(Cs)
    idx, sc = ctx.best_match(measure, qo, qv, co, cv, k, min_score)
    return np.where(idx == 0xFFFFFFFF, -1, idx.astype(np.int64)), sc


def _same(got, exp):
    gi, gs = got
    ei, es = exp
    assert gi.shape == ei.shape
    bad = np.argwhere(gi != ei)
    assert bad.size == 0, "index differs at %s: got %s expected %s" % (bad[:5].tolist(), gi[tuple(bad[0])], ei[tuple(bad[0])])
    assert np.array_equal(gs.view(np.uint64), es.view(np.uint64)) or np.array_equal(gs, es, equal_nan=True)
    nan = np.isnan(es)
    assert np.array_equal(np.isnan(gs), nan)
    assert np.array_equal(gs[~nan].view(np.uint64), es[~nan].view(np.uint64))


def _check(ctx, measure, Q, Cs, k, min_score=None):
    got = _run(ctx, measure, Q, Cs, k, min_score)
    exp = R.topk(R.score_matrix(measure, Q, Cs), k, min_score)
    _same(got, exp)
    return got


def _strings(seed, n, alphabet=gen.ASCII_LOWER, lo=0, hi=32):
    A, B = gen.pairs(seed, (n + 1) // 2, alphabet, lo, hi)
    return (A + B)[:n]


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65])
def test_small_frames(ctx, measure, k, m):
    Q = _strings(10 + m, 64)
    Cs = _strings(20 + m, m, "abcde", 0, 12)  # small alphabet: many ties
    _check(ctx, measure, Q, Cs, k)


@pytest.mark.parametrize("measure", MEASURES)
def test_one_query_five_thousand_candidates(ctx, measure):
    _check(ctx, measure, _strings(3, 1), _strings(4, 5000), 16)
    _check(ctx, measure, _strings(5, 64), _strings(6, 5000, "abcd", 0, 10), 3)


@pytest.mark.parametrize("measure", MEASURES)
def test_ten_thousand_queries(ctx, measure):
    _check(ctx, measure, _strings(7, 10000), _strings(8, 64), 3)


@pytest.mark.parametrize("measure", MEASURES)
def test_min_score_at_below_and_above_an_achieved_score(ctx, measure):
    Q, Cs = _strings(30, 64), _strings(31, 65, "abcdef", 0, 10)
    sc = R.score_matrix(measure, Q, Cs)
    s = float(np.median(sc))
    for ms in (s, np.nextafter(s, -1.0), np.nextafter(s, 2.0), 0.0, -np.inf, 1.0):
        _check(ctx, measure, Q, Cs, 16, ms)


@pytest.mark.parametrize("measure", MEASURES)
def test_empty_strings_duplicates_and_all_equal(ctx, measure):
    Q = ["", "a", "abc", "abcabc", "", "zz"] * 11
    _check(ctx, measure, Q, ["abc", "", "abc", "ab", "", "abc", "x" * 32], 16)
    _check(ctx, measure, Q, ["same"] * 70, 16)
    _check(ctx, measure, Q, ["", "", ""], 4)


def _edge_strings(seed):
    rng = random.Random(seed)
    out = []
    for n in (31, 32, 33):
        out += ["".join(rng.choice("abcxyz") for _ in range(n)) for _ in range(4)]
    out += ["cafés", "naïve", "日本語テキスト", "Привет мир", "abc" + "é" * 15, "x" * 31 + "é"]
    out += ["".join(rng.choice("abcdef") for _ in range(1500)), "q" * 1100 + "abc"]
    out += _strings(seed, 20)
    return out


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("k", [1, 16])
def test_lengths_around_32_non_ascii_and_long_strings(ctx, measure, k):
    E = _edge_strings(41)
    F = _strings(42, 70)
    _check(ctx, measure, E, F, k)         # slow queries x fast candidates
    _check(ctx, measure, F, E, k)         # fast queries x slow candidates
    _check(ctx, measure, E, E[::-1], k)   # slow x slow


@pytest.mark.parametrize("side", ["queries", "candidates", "both"])
@pytest.mark.parametrize("k", [1, 3])
def test_more_slow_strings_than_one_batch(ctx, side, k):
    # 37 slow queries and 21 slow candidates (gen.batch_boundary_frame): the fallback folds three batches of slow queries and
    # two of slow candidates into its list
    Q, Cs = gen.batch_boundary_frame(171, side)
    for measure in MEASURES:
        _check(ctx, measure, Q, Cs, k)


@pytest.mark.parametrize("measure", ["levenshtein", "jaro_winkler"])
def test_candidate_split_and_merge_20k(ctx, measure):
    # 20 k x 20 k: the candidates are split over many workgroups and merged; 200 of the queries are held to the oracle
    Q, Cs = _strings(50, 20000, "abcdefgh", 0, 16), _strings(51, 20000, "abcdefgh", 0, 16)
    gi, gs = _run(ctx, measure, Q, Cs, 16)
    rows = np.random.default_rng(0).choice(len(Q), 200, replace=False)
    exp = R.topk(R.score_matrix(measure, [Q[i] for i in rows], Cs), 16)
    _same((gi[rows], gs[rows]), exp)


@pytest.mark.parametrize("measure", MEASURES)
def test_scores_are_what_the_pairwise_path_returns(ctx, measure):
    # every reported (query, candidate) score equals strsim_pairs_host of that pair, bit for bit, on a mixed 256 x 4096 frame
    Q = _strings(60, 240) + _edge_strings(61)[:16]
    Cs = _strings(62, 4096)
    gi, gs = _run(ctx, measure, Q, Cs, 16)
    sel = gi >= 0
    ii = np.nonzero(sel)[0]
    jj = gi[sel]
    A = [Q[i] for i in ii]
    B = [Cs[j] for j in jj]
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    pw = ctx.pairs_host(measure, ao, av, bo, bv)
    assert np.array_equal(pw.view(np.uint64), gs[sel].view(np.uint64))


def test_python_nulls_and_index_remap(ctx):
    Q = ["abc", None, "abd", "zzz"]
    Cs = [None, "abd", None, "abc", "zz"]
    idx, sc = S.best_match("levenshtein", Q, Cs, k=3, ctx=ctx)
    exp_i, exp_s = R.topk(R.score_matrix("levenshtein", ["abc", "", "abd", "zzz"], ["abd", "abc", "zz"]), 3)
    pos = np.array([1, 3, 4])
    exp_i = np.where(exp_i >= 0, pos[np.maximum(exp_i, 0)], -1)
    exp_i[1] = -1
    exp_s[1] = np.nan
    assert np.array_equal(idx, exp_i)
    assert np.array_equal(sc, exp_s, equal_nan=True)
    assert idx[0, 0] == 3 and sc[0, 0] == 1.0


# Fast-class strings beyond a-z: capitals, digits, space and punctuation vary bits 5 and 6 of the bytes, so the lane kernel
# must take its seven-bit-plane match masks.  A wave of queries that mixes lowercase-only strings with mixed ones, and
# mixed-case candidates against lowercase-only queries, exercise the choice between five and seven planes from both sides.
MIXED_ASCII = "abcdeABCDE019 .-_'@XYZxyz"


def _mixed(seed, n, alphabet=MIXED_ASCII, lo=0, hi=32):
    rng = random.Random(seed)
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("k", [1, 16])
def test_mixed_ascii_seven_planes(ctx, measure, k):
    lower = _strings(70, 200, "abcde", 0, 20)
    mixed = _mixed(71, 200, lo=1, hi=32)
    # queries: waves (64 lanes) alternating lowercase-only / mixed / interleaved
    Q = lower[:64] + mixed[:64] + [x for pair in zip(lower[64:96], mixed[64:96]) for x in pair] + mixed[100:140]
    cand_mixed = _mixed(72, 150, lo=0, hi=32) + ["aBcDe", "ABCDE", "abcde", "a-b c", "A", "a", "0", " "]
    cand_lower = _strings(73, 120, "abcde", 0, 20)
    _check(ctx, measure, Q, cand_mixed, k)              # every kind of query wave against mixed candidates
    _check(ctx, measure, lower[:64], cand_mixed, k)     # lowercase-only queries, mixed-case candidates
    _check(ctx, measure, mixed[:64], cand_lower, k)     # mixed queries, lowercase-only candidates


@pytest.mark.parametrize("measure", MEASURES)
def test_case_is_not_ignored(ctx, measure):
    # 'a' and 'A' differ only in bit 5: a wrong plane choice would score "abc" / "ABC" as equal
    Q = ["abc"] * 64 + ["ABC"] * 64
    Cs = ["ABC", "abc", "aBc", "AbC"]
    got = _check(ctx, measure, Q, Cs, 4)
    assert (got[0][:64, 0] == 1).all() and (got[0][64:, 0] == 0).all()
