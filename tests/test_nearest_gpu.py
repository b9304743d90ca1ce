"""Nearest match on the MI355X (strsim_nearest_*) against the contract stated independently: distance_ref's edit distance of every
pair, then a NumPy top-k (tests/nearest_ref.py) -- ascending distance, ties to the lower candidate index, the cutoff applied."""
import random

import numpy as np
import pytest

import gen
import nearest_ref as R

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")
MEASURES = ("levenshtein", "osa")
U = R.UNBOUNDED


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def _run(ctx, measure, Q, Cs, k, md=None):
    qo, qv = S.pack_strings(Q)
    co, cv = S.pack_strings(Cs)
    idx, dist = ctx.nearest(measure, qo, qv, co, cv, k, md)
    empty = idx == 0xFFFFFFFF
    assert np.array_equal(empty, dist == 0xFFFFFFFF)
    return np.where(empty, -1, idx.astype(np.int64)), np.where(empty, -1, dist.astype(np.int64))


def _same(got, exp, rows=None):
    gi, gd = got
    ei, ed = exp
    if rows is not None:
        gi, gd = gi[rows], gd[rows]
    assert gi.shape == ei.shape
    bad = np.argwhere((gi != ei) | (gd != ed))
    assert bad.size == 0, "row %d differs: got %s / %s, expected %s / %s" % (
        bad[0][0], gi[bad[0][0]].tolist(), gd[bad[0][0]].tolist(), ei[bad[0][0]].tolist(), ed[bad[0][0]].tolist())


def _check(ctx, measure, Q, Cs, k, md=None):
    got = _run(ctx, measure, Q, Cs, k, md)
    _same(got, R.topk(R.distance_matrix(measure, Q, Cs), k, md))
    return got


def _strings(seed, n, alphabet=gen.ASCII_LOWER, lo=0, hi=32):
    A, B = gen.pairs(seed, (n + 1) // 2, alphabet, lo, hi)
    return (A + B)[:n]


def _near_duplicates(seed, cands, n, alphabet=gen.ASCII_LOWER):
    """frame (b): each query a random candidate with 0..3 random edits (insert, delete, substitute, adjacent swap)"""
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


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("md", [0, 1, 2, 5, None])
def test_nearest_gpu_random_ascii(ctx, measure, k, md):
    Q = _strings(11, 300, lo=0, hi=12)
    Cs = _strings(12, 500, lo=0, hi=12)
    _check(ctx, measure, Q, Cs, k, md)


@pytest.mark.parametrize("measure", MEASURES)
def test_nearest_gpu_edge_lengths(ctx, measure):
    # 0, 1, 31, 32 take the lane path, 33 the fallback; near copies across the lengths
    rng = random.Random(5)
    base = "".join(rng.choice("abcd") for _ in range(33))
    Q = [base[:n] for n in (0, 1, 31, 32, 33)] + [base[1:32], base[:30] + "zz", "", "a"]
    Cs = [base[:n] for n in (0, 1, 2, 30, 31, 32, 33)] + [base[2:33], base[:31] + "x", "b", ""]
    for k in (1, 3, 16):
        for md in (0, 1, 2, None):
            _check(ctx, measure, Q, Cs, k, md)


@pytest.mark.parametrize("measure", MEASURES)
def test_nearest_gpu_heavy_ties(ctx, measure):
    # duplicate candidates and a two-letter alphabet: many equal distances, decided by the index
    Q = _strings(21, 400, alphabet="ab", lo=0, hi=10)
    base = _strings(22, 60, alphabet="ab", lo=0, hi=10)
    Cs = base + base[::-1] + base
    for k in (1, 3, 16):
        for md in (1, None):
            _check(ctx, measure, Q, Cs, k, md)


@pytest.mark.parametrize("measure", MEASURES)
def test_nearest_gpu_empty_candidates_and_k_above_rows(ctx, measure):
    Q = ["abc", "", "xyz"]
    gi, gd = _run(ctx, measure, Q, [], 3)
    assert (gi == -1).all() and (gd == -1).all()
    _check(ctx, measure, Q, ["ab", "abcd"], 16)
    _check(ctx, measure, Q, ["ab", "abcd"], 16, 1)
    gi, gd = _run(ctx, measure, [], ["a"], 4)
    assert gi.shape == (0, 4)


@pytest.mark.parametrize("measure", MEASURES)
def test_nearest_gpu_mixed_case_five_and_seven_planes(ctx, measure):
    # a wave of lowercase queries runs five planes against lowercase candidates and seven against mixed-case ones
    Q = _strings(31, 256, lo=1, hi=16) + _strings(32, 128, alphabet="abcXYZ09 -", lo=1, hi=16)
    Cs = _strings(33, 300, lo=1, hi=16) + _strings(34, 100, alphabet="aBcXyZ09_ ", lo=1, hi=16) + ["HELLO", "hello", "Hello"]
    for k in (1, 16):
        _check(ctx, measure, Q, Cs, k)
        _check(ctx, measure, Q, Cs, k, 2)


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("side", ["queries", "candidates", "both"])
def test_nearest_gpu_slow_strings(ctx, measure, side):
    # non-ASCII and > 32-byte strings go through strsim_distance_device, scored once per pair
    fast_q = _strings(41, 150, lo=0, hi=20)
    fast_c = _strings(42, 120, lo=0, hi=20)
    slow_q = ["héllo wörld", "日本語テキスト", "x" * 40, "kitten" * 6, "ab" * 17, "ñ"]
    slow_c = ["hello world", "héllo wörld", "y" * 33, "kitten" * 6 + "s", "日本語", "ab" * 17, "n"]
    Q = fast_q + (slow_q if side in ("queries", "both") else [])
    Cs = fast_c + (slow_c if side in ("candidates", "both") else []) + ["hello world"]
    rng = random.Random(43)
    rng.shuffle(Q)
    rng.shuffle(Cs)
    for k in (1, 3, 16):
        for md in (2, None):
            _check(ctx, measure, Q, Cs, k, md)


@pytest.mark.parametrize("side", ["queries", "candidates", "both"])
@pytest.mark.parametrize("k", [1, 3])
def test_nearest_gpu_more_slow_strings_than_one_batch(ctx, side, k):
    # 37 slow queries and 21 slow candidates (gen.batch_boundary_frame): the fallback folds three batches of slow queries and
    # two of slow candidates into its list
    Q, Cs = gen.batch_boundary_frame(181, side)
    for measure in MEASURES:
        for md in (3, None):
            _check(ctx, measure, Q, Cs, k, md)


@pytest.mark.parametrize("measure", MEASURES)
def test_nearest_gpu_near_duplicates_dynamic_bound(ctx, measure):
    # frame (b) small: most queries have a candidate within 3 edits, so the bound of a full list cuts the sweep short
    Cs = _strings(51, 1000, lo=4, hi=24)
    Q = _near_duplicates(52, Cs, 3000)
    for md in (None, 2):
        got = _check(ctx, measure, Q, Cs, 1, md)
        if md is None:  # (each edit costs at most 2: an adjacent swap is two Levenshtein edits)
            assert (got[1][:, 0] <= 6).all() and (got[1][:, 0] <= 2).mean() > 0.5
    _check(ctx, measure, Q[:500], Cs, 4)


def _sample_check(ctx, measure, Q, Cs, k, md, rows):
    got = _run(ctx, measure, Q, Cs, k, md)
    exp = R.topk(R.distance_matrix(measure, [Q[i] for i in rows], Cs), k, md)
    _same(got, exp, rows)


@pytest.mark.parametrize("measure", MEASURES)
def test_nearest_gpu_split_frame_few_queries(ctx, measure):
    # 2 k queries x 200 k candidates: few query waves, so the candidates are split over grid.y and the lists merged
    Q = _strings(61, 2000, lo=0, hi=32)
    Cs = _strings(62, 200_000, lo=0, hi=32)
    rows = np.random.default_rng(63).choice(len(Q), 6, replace=False)
    _sample_check(ctx, measure, Q, Cs, 3, None, rows)
    _sample_check(ctx, measure, Q, Cs, 1, 2, rows)


def test_nearest_gpu_split_frame_square(ctx):
    Q = _strings(71, 20_000, lo=0, hi=32)
    Cs = _near_duplicates(72, Q[:5000], 20_000)
    rows = np.random.default_rng(73).choice(len(Q), 16, replace=False)
    _sample_check(ctx, "levenshtein", Q, Cs, 16, None, rows)
    _sample_check(ctx, "osa", Q, Cs, 1, 1, rows)


@pytest.mark.parametrize("measure", MEASURES)
def test_nearest_gpu_permuted_candidates_map_back(ctx, measure):
    # the same search over a permuted candidate column: the same distances row by row, each answer maps back (through the
    # permutation) to a candidate at that distance, and the lists are exactly the reference's for the permuted order
    Q = _strings(81, 500, lo=0, hi=14)
    Cs = _strings(82, 700, lo=0, hi=14) + ["Zürich", "z" * 35]
    perm = np.random.default_rng(83).permutation(len(Cs))
    Dm = R.distance_matrix(measure, Q, Cs)
    a_i, a_d = _run(ctx, measure, Q, Cs, 16, 3)
    b_i, b_d = _run(ctx, measure, Q, [Cs[j] for j in perm], 16, 3)
    assert np.array_equal(a_d, b_d)
    I, J = np.nonzero(b_i >= 0)
    assert np.array_equal(Dm[I, perm[b_i[I, J]]], b_d[I, J])
    _same((b_i, b_d), R.topk(Dm[:, perm], 16, 3))


def test_nearest_gpu_repeatable(ctx):
    Q = _strings(91, 5000, alphabet="abc", lo=0, hi=12)
    Cs = _strings(92, 3000, alphabet="abc", lo=0, hi=12)
    for measure in MEASURES:
        a = _run(ctx, measure, Q, Cs, 16)
        b = _run(ctx, measure, Q, Cs, 16)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("measure", MEASURES)
def test_nearest_gpu_agrees_with_distance_calls(ctx, measure):
    # every reported (i, j, d) is what strsim_distance_device returns for that pair
    Q = _strings(101, 200, lo=0, hi=20) + ["héllo", "q" * 40]
    Cs = _strings(102, 300, lo=0, hi=20) + ["hello", "q" * 39]
    gi, gd = _run(ctx, measure, Q, Cs, 16, 4)
    I, J = np.nonzero(gi >= 0)
    jj = gi[I, J]
    qo, qv = S.pack_strings([Q[i] for i in I])
    co, cv = S.pack_strings([Cs[j] for j in jj])
    d = ctx.distance_host(measure, qo, qv, co, cv)
    assert np.array_equal(d.astype(np.int64), gd[I, J])


def test_nearest_gpu_python_wrapper_nulls(ctx):
    Q = ["kitten", None, "abc", "zzzz"]
    Cs = [None, "sitting", "abd", None, "kitten"]
    idx, dist = S.nearest("levenshtein", Q, Cs, k=2, max_distance=3, ctx=ctx)
    assert idx.tolist() == [[4, 1], [-1, -1], [2, -1], [-1, -1]]
    assert dist.tolist() == [[0, 3], [-1, -1], [1, -1], [-1, -1]]
    idx, dist = S.nearest("osa", ["ab"], ["ba", "ab"], ctx=ctx)
    assert idx.tolist() == [[1]] and dist.tolist() == [[0]]
