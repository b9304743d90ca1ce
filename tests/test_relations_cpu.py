"""The licence of tests/test_relations_gpu.py: every relation of tests/relation_checks.py holds on the oracle and the *_ref models,
over the frames the GPU tests use (tests/relation_frames.py), so a relation that fails on the GPU points at a kernel and not at the
mathematics.  Also the generator's own conditions: scores that are not degenerate, cutoffs that cut.

Relation x measure cells that are NOT asserted, here or on the GPU:
  * reversal for jaro / jaro_winkler (their greedy matching is not reversal-invariant) and for partial_ratio (its tie rules are not);
  * swap for partial_ratio's spans (they swap roles except on ties): the score alone is compared;
  * token_set_ratio >= token_sort_ratio: false (for instance "a b" / "a c": the set form scores sect + ab against sect + ba).
Every other cell of the issue's table holds on the models: nothing was dropped for failing here.
"""
import numpy as np
import pytest

import relation_checks as RC
import relation_frames as F
import relations as T

N_LONG_CPU = 60  # the 1 024 / 1 025-character affix cases: a million DP cells a pair on the CPU


@pytest.fixture(scope="module")
def be():
    return RC.ModelBackend()


# ---- the transformations themselves ----

def test_relabel_is_injective_monotone_and_keeps_whitespace():
    s = "".join(chr(c) for c in range(1, 128))
    for base in T.RELABEL_BASES:
        img = T.relabel(s, base)
        assert len(img) == len(s) and T.unrelabel(img, base) == s
        assert [c.isspace() for c in img] == [c.isspace() for c in s]
        body = [c for c in img if not c.isspace()]
        assert body == sorted(body) and len(set(body)) == len(body)
        assert all(len(c.encode()) == {0x400: 2, 0x4E00: 3, 0x1F600: 4}[base] for c in body)
        assert sorted("ab b a ba".split()) == [T.unrelabel(t, base) for t in sorted(T.relabel("ab b a ba", base).split())]


def test_base_pairs_are_lane_class_and_padded_pairs_sit_at_the_caps():
    for A, B in (F.pair_frame(), F.token_frame(), F.equal_length_frame()):
        assert all(s.isascii() and len(s) <= T.BASE_MAX_LEN for s in A + B)
    assert sum(not a for a in F.pair_frame()[0]) > 20 and sum(a == b for a, b in zip(*F.pair_frame())) > 100
    for m, caps in T.AFFIX_CAPS.items():
        for cap in caps:
            for longest in (cap, cap + 1):
                A, B = F.padded_frame(longest, 50)
                assert all(max(len(a), len(b)) == longest and a.isascii() and b.isascii() for a, b in zip(A, B))
    needles, hay = F.contained_frame()
    assert all(a and a in h for a, h in zip(needles, hay))
    assert {len(h) for h in hay} == set(F.HAYSTACK_LENGTHS)


def test_token_images_keep_the_tokens_and_leave_the_lane_tier():
    A, B = F.token_frame()
    for mode in ("spread", "unicode", "copies"):
        A2, _ = F.token_images(mode, "a")
        _, B2 = F.token_images(mode, "b")
        for X, X2 in ((A, A2), (B, B2)):
            if mode == "copies":
                assert all(sorted(s.split() * 4) == sorted(t.split()) for s, t in zip(X, X2))
                assert max(len(t.split()) for t in X2) > 16 and min(len(t.split()) for t in X2 if t.split()) <= 16
            else:
                assert all(sorted(s.split()) == sorted(t.split()) for s, t in zip(X, X2))
            if mode == "spread":
                assert all(t.isascii() and len(t) > 64 for t in X2)
            if mode == "unicode":
                assert sum(not t.isascii() for t in X2) > len(X2) // 2
    assert any(s != s.strip() for s in F.token_images("unicode", "a")[0])  # leading and trailing runs


# ---- the generator's conditions, on the models' output ----

@pytest.mark.parametrize("m", RC.SIMILARITIES)
def test_scores_are_not_degenerate(be, m):
    A, B = F.token_frame() if m in RC.TOKEN else F.pair_frame()
    s = be.sim(m, A, B)
    share = float(((s == 0.0) | (s == 1.0)).mean())
    print(m, "share of scores that are exactly 0.0 or 1.0:", share)
    assert share <= 0.30


@pytest.mark.parametrize("m", RC.DISTANCES)
def test_cutoffs_cut(be, m):
    A, B = F.pair_frame()
    d = be.dist(m, A, B, None)
    for k in RC.CUTOFFS[m]:
        above = float((d > k).mean())
        print(m, "k =", k, "share above:", above)
        assert above >= 0.25 and 1.0 - above >= 0.25
        assert np.array_equal(be.dist(m, A, B, k), np.minimum(d, k + 1))
    assert np.array_equal(be.dist(m, A, B, 0), np.minimum(d, 1))


def _cuts(values, keep):
    """Some query has a candidate the cutoff drops and one it keeps."""
    return bool((keep.any(axis=1) & (~keep).any(axis=1)).any())


def test_search_cutoffs_cut(be):
    Q, Cs = F.search_frame()
    for m in ("levenshtein", "osa"):
        d = be.NR.distance_matrix(m, Q[:32], Cs)
        assert _cuts(d, d <= F.NEAREST_CUTOFF)
    s = be.EX.score_matrix("ratio", Q[:32], Cs)
    assert _cuts(s, s >= F.EXTRACT_CUTOFF["indel"])
    TQ, TC = F.token_search_frame()
    s = be.EX.score_matrix("token_sort_ratio", TQ[:32], TC)
    assert _cuts(s, s >= F.EXTRACT_CUTOFF["token_sort_ratio"])
    for m in RC.CLASSIC:
        s = be.BM.score_matrix(m, Q[:32], Cs)
        assert _cuts(s, s >= F.BEST_MATCH_CUTOFF[m]), m


# ---- the relations ----

@pytest.mark.parametrize("base", T.RELABEL_BASES)
@pytest.mark.parametrize("m", RC.SIMILARITIES)
def test_relabel_similarity_cpu(be, m, base):
    RC.relabel_sim(be, m, base, *(F.token_frame() if m in RC.TOKEN else F.pair_frame()))


@pytest.mark.parametrize("base", T.RELABEL_BASES)
@pytest.mark.parametrize("m", RC.DISTANCES)
def test_relabel_distance_cpu(be, m, base):
    RC.relabel_dist(be, m, base, *F.pair_frame())


@pytest.mark.parametrize("base", T.RELABEL_BASES)
def test_relabel_partial_alignment_and_token_sort_cpu(be, base):
    RC.relabel_partial(be, base, *F.pair_frame())
    A, B = F.token_frame()
    RC.relabel_token_sort(be, base, A + B + F.token_images("unicode", "a")[0])


@pytest.mark.parametrize("m,cap", [(m, cap) for m, caps in T.AFFIX_CAPS.items() for cap in caps])
def test_common_affix_distance_cpu(be, m, cap):
    n = N_LONG_CPU if cap >= 1024 else 1000
    A, B = F.pair_frame()
    for longest in (cap, cap + 1):
        RC.affix_dist(be, m, A[:n], B[:n], *F.padded_frame(longest, n), what=f"padded to {longest} bytes")


@pytest.mark.parametrize("m", RC.DISTANCES)
def test_non_ascii_prefix_distance_cpu(be, m):
    A, B = F.pair_frame()
    RC.affix_dist(be, m, A, B, ["é" + a for a in A], ["é" + b for b in B], what="behind a non-ASCII prefix")


@pytest.mark.parametrize("kind,m", [("dist", m) for m in RC.DISTANCES] + [("sim", m) for m in RC.REVERSAL_SIMS])
def test_reversal_cpu(be, kind, m):
    RC.reversal(be, kind, m, *F.pair_frame())


@pytest.mark.parametrize("kind,m", [("dist", m) for m in RC.DISTANCES] + [("sim", m) for m in RC.SWAP_SIMS])
def test_swap_cpu(be, kind, m):
    RC.swap(be, kind, m, *(F.token_frame() if m in RC.TOKEN else F.pair_frame()))


def test_distance_order_cpu(be):
    lev, osa, ind = RC.distance_order(be, *F.pair_frame())
    assert (osa < lev).mean() > 0.02 and (lev < ind).mean() > 0.3  # the three really differ on this frame


def test_partial_ratio_relations_cpu(be):
    assert RC.partial_spans_are_indel(be, *F.pair_frame()) > 0.9 * F.N
    RC.partial_contained(be, *F.contained_frame())
    RC.partial_at_least_indel(be, *F.equal_length_frame())


@pytest.mark.parametrize("m,mode", [(m, mode) for m in RC.TOKEN for mode in ("spread", "unicode")] + [("token_set_ratio", "copies")])
def test_token_invariance_cpu(be, m, mode):
    A, B = F.token_frame()
    for side in ("a", "b"):
        RC.token_invariance(be, m, A, B, *F.token_images(mode, side), what=f"with side {side} permuted ({mode})")


def test_token_sort_relations_cpu(be):
    A, B = F.token_frame()
    A2, B2 = F.token_images("unicode", "a")[0], F.token_images("spread", "b")[1]
    assert RC.token_sort_idempotent(be, A + A2 + B2) == [" ".join(sorted(s.split())) for s in A + A2 + B2]
    RC.token_sort_ratio_is_indel(be, A, B)
    RC.token_sort_ratio_is_indel(be, A2, B2)


@pytest.mark.parametrize("kind,m", [("sim", m) for m in RC.SIMILARITIES] + [("dist", m) for m in RC.DISTANCES])
def test_batch_relations_cpu(be, kind, m):
    """(Row-wise models satisfy these by construction; this holds the checks' own index arithmetic.)"""
    A, B = (x[:600] for x in (F.token_frame() if m in RC.TOKEN else F.pair_frame()))
    k = RC.CUTOFFS[m][1] if kind == "dist" else None
    RC.batch_permutation(be, kind, m, A, B, k, 9)
    RC.batch_concatenation(be, kind, m, A[:300], B[:300], [T.relabel(s, 0x400) for s in A[300:]], [T.relabel(s, 0x1F600) for s in B[300:]], k)
    RC.batch_literal(be, kind, m, A[:300], B[7], k)


@pytest.mark.parametrize("m", ("levenshtein", "osa"))
def test_search_nearest_cpu(be, m):
    Q, Cs = (x[:n] for x, n in zip(F.search_frame(), (32, 100)))
    for k in F.SEARCH_KS:
        for md in (F.NEAREST_CUTOFF, None):
            RC.search_invariance(be, "nearest", m, Q, Cs, [T.relabel(s, 0x4E00) for s in Q], [T.relabel(s, 0x4E00) for s in Cs], k, md, "relabelled")
            RC.search_invariance(be, "nearest", m, Q, Cs, [F.SEARCH_PREFIX + s for s in Q], [F.SEARCH_PREFIX + s for s in Cs], k, md, "prefixed")


@pytest.mark.parametrize("scorer", ("indel", "token_sort_ratio"))
def test_search_extract_cpu(be, scorer):
    Q, Cs = (x[:n] for x, n in zip(F.token_search_frame() if scorer == "token_sort_ratio" else F.search_frame(), (32, 100)))
    for k in F.SEARCH_KS:
        for cut in (F.EXTRACT_CUTOFF[scorer], None):
            RC.search_invariance(be, "extract", scorer, Q, Cs, [T.relabel(s, 0x400) for s in Q], [T.relabel(s, 0x400) for s in Cs], k, cut, "relabelled")


@pytest.mark.parametrize("m", RC.CLASSIC)
def test_search_best_match_cpu(be, m):
    Q, Cs = (x[:n] for x, n in zip(F.search_frame(), (32, 100)))
    for k in F.SEARCH_KS:
        for cut in (F.BEST_MATCH_CUTOFF[m], None):
            RC.search_invariance(be, "best_match", m, Q, Cs, [T.relabel(s, 0x400) for s in Q], [T.relabel(s, 0x400) for s in Cs], k, cut, "relabelled")
