"""The match_join_<measure> plugin functions end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host).  Expected values: the hits of tests/match_join_ref.py over the non-null candidates, mapped back to their
rows of input 1; a null list for a null query.  Scores are compared bit for bit."""
import numpy as np
import pyarrow as pa
import pytest

import gen
import match_join_ref as R

pytestmark = pytest.mark.gpu
MEASURES = R.MEASURES
LIST = pa.large_list(pa.field("item", pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])))


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def min_score(v):
    return [pa.array([v], type=pa.float64())]


def _check(got, measure, Q, Cs, cut=None):
    """the one chunk of a result against the model: offsets, list validity, indices and scores"""
    n = len(Q)
    assert got.type == LIST and got.num_chunks == 1 and len(got) == n
    arr = got.chunk(0)
    pos = [j for j, c in enumerate(Cs) if c is not None]
    ep, ei, es = R.join(measure, [q if q is not None else "" for q in Q], [Cs[j] for j in pos], cut)
    counts = np.where([q is not None for q in Q], np.diff(ep.astype(np.int64)), 0)
    assert arr.offsets.to_pylist() == [0] + np.cumsum(counts).tolist()
    assert np.asarray(arr.is_valid()).tolist() == [q is not None for q in Q]
    keep = np.repeat(np.array([q is not None for q in Q], dtype=bool), np.diff(ep.astype(np.int64)))
    flat = arr.values
    assert flat.null_count == 0 and len(flat) == int(keep.sum())
    index = flat.field("index").to_numpy(zero_copy_only=False)
    score = flat.field("score").to_numpy(zero_copy_only=False)
    assert np.array_equal(index, np.array(pos, dtype=np.int64)[ei.astype(np.int64)][keep] if len(pos) else np.zeros(0))
    assert np.array_equal(np.ascontiguousarray(score).view(np.uint64), es[keep].view(np.uint64))


@pytest.mark.parametrize("measure", MEASURES)
def test_match_join_plugin_list_of_struct_result_and_name(H, measure):
    A, B = gen.pairs(181, 70, gen.ASCII_LOWER, 0, 10)
    Q, Cs = A, B[:40] + A[:10]
    probe = {}
    got = H.call_plugin("match_join_" + measure, Q, Cs, names=("query", "cands"), _probe=probe, out_type=LIST, extra=min_score(0.6))
    assert probe["name"] == "query"
    assert probe["series_released"] == [1, 1, 1] and probe["arrays_released"] == [True, True, True]
    _check(got, measure, Q, Cs, 0.6)
    row = got.to_pylist()[3]
    assert {"index": 43, "score": 1.0} in row and [h["index"] for h in row] == sorted(h["index"] for h in row)


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("layout", ["vu", ("u", "vu")])
def test_match_join_plugin_nulls_both_sides_and_min_score(H, measure, layout):
    A, B = gen.pairs(183, 120, gen.ASCII_LOWER, 0, 12)
    Q = [None if i % 7 == 3 else a for i, a in enumerate(A)]
    Cs = [None if j % 5 == 1 else b for j, b in enumerate(B[:43])] + ["Привет мир", "x" * 40] + A[:6]
    qa = pa.chunked_array([pa.array(Q[:50]), pa.array(Q[50:51]), pa.array(Q[51:])])
    ca = pa.chunked_array([pa.array(Cs[:20]), pa.array(Cs[20:])])
    got = H.call_plugin("match_join_" + measure, qa, ca, layout=layout, out_type=LIST)  # min_score absent: every pair
    _check(got, measure, Q, Cs)
    assert got.null_count == sum(q is None for q in Q)
    rows = got.to_pylist()
    assert rows[3] is None and len(rows[0]) == sum(c is not None for c in Cs) and all(h["index"] % 5 != 1 or h["index"] >= 43 for h in rows[0])
    # a null min_score is no cutoff
    _check(H.call_plugin("match_join_" + measure, qa, ca, layout=layout, out_type=LIST, extra=[pa.array([None], type=pa.float64())]), measure, Q, Cs)
    for cut in (0.0, 0.6, 1.0, 1.5):
        _check(H.call_plugin("match_join_" + measure, qa, ca, layout=layout, out_type=LIST, extra=min_score(cut)), measure, Q, Cs, cut)


def test_match_join_plugin_empty_sides_and_all_candidates_null(H):
    got = H.call_plugin("match_join_jaro", ["a", None, "b"], [None, None], out_type=LIST)
    assert got.to_pylist() == [[], None, []]
    got = H.call_plugin("match_join_levenshtein", ["a", None], pa.array([], type=pa.string()), out_type=LIST)
    assert got.to_pylist() == [[], None]
    got = H.call_plugin("match_join_jaccard", pa.array([], type=pa.string()), ["a"], out_type=LIST)
    assert got.to_pylist() == [] and got.type == LIST
    got = H.call_plugin("match_join_jaro_winkler", ["ab", "abc"], ["ba", "ab"], out_type=LIST, extra=min_score(1.5))
    assert got.to_pylist() == [[], []]
    got = H.call_plugin("match_join_levenshtein", ["ab", "abcd"], ["ba", "ab"], out_type=LIST, extra=min_score(0.5))
    assert got.to_pylist() == [[{"index": 1, "score": 1.0}], [{"index": 1, "score": 0.5}]]
    got = H.call_plugin("match_join_sorensen_dice", ["ab"], ["ba", "xy"], out_type=LIST, extra=min_score(1.0))
    assert got.to_pylist() == [[{"index": 0, "score": 1.0}]]


def test_match_join_plugin_bad_min_score(H):
    # the third input is parsed as join's score_cutoff, and its messages say so
    Q, Cs = ["abc", "abd"], ["abd", "xyz", "q"]
    bad = [
        ([pa.array([0.5, 0.6], type=pa.float64())], "score_cutoff must be a single value"),
        ([pa.array([float("nan")], type=pa.float64())], "score_cutoff must not be NaN"),
        ([pa.array([1], type=pa.int64())], "score_cutoff must be a Float64"),
        ([pa.array([1], type=pa.uint32())], "score_cutoff must be a Float64"),
    ]
    for m in MEASURES:
        for extra, words in bad:
            with pytest.raises(H.PluginError, match=words):
                H.call_plugin("match_join_" + m, Q, Cs, out_type=LIST, extra=extra)
        with pytest.raises(H.PluginError, match="join: expected 2 input series"):
            H.call_plugin("match_join_" + m, Q, Cs, out_type=LIST, extra=min_score(0.5) + min_score(0.6))
