"""The qgram_join_<kind> and qgram_cluster_<kind> plugin functions end to end on the GPU, with pyarrow standing in for the Polars
engine (strsim_amd.arrow_host).  Expected values: the hits of tests/qgram_join_ref.py over the non-null candidates, mapped back to
their rows of input 1, a null list for a null query; the roots of tests/cluster_ref.py over the non-null rows, null for a null
row.  Scores are compared bit for bit."""
import numpy as np
import pyarrow as pa
import pytest

import cluster_ref
import qgram_join_frames as F
import qgram_join_ref as R

pytestmark = pytest.mark.gpu
KINDS = R.KINDS
LIST = pa.large_list(pa.field("item", pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])))
U32 = pa.uint32()


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def u32(v):
    return pa.array([v], type=pa.uint32())


def f64(v):
    return pa.array([v], type=pa.float64())


def mode(q, multiset):
    return [u32(q), u32(0 if multiset else 1)]


def _check(got, kind, q, multiset, Q, Cs, cut=None):
    """the one chunk of a result against the model: offsets, list validity, indices and scores"""
    n = len(Q)
    assert got.type == LIST and got.num_chunks == 1 and len(got) == n
    arr = got.chunk(0)
    pos = [j for j, c in enumerate(Cs) if c is not None]
    ep, ei, es = R.join(kind, [s if s is not None else "" for s in Q], [Cs[j] for j in pos], cut, q, multiset)
    valid = np.array([s is not None for s in Q], dtype=bool)
    counts = np.where(valid, np.diff(ep.astype(np.int64)), 0)
    assert 0 < counts.sum() < valid.sum() * len(pos) or cut is None
    assert arr.offsets.to_pylist() == [0] + np.cumsum(counts).tolist()
    assert np.asarray(arr.is_valid()).tolist() == valid.tolist()
    keep = np.repeat(valid, np.diff(ep.astype(np.int64)))
    flat = arr.values
    assert flat.null_count == 0 and len(flat) == int(keep.sum())
    index = flat.field("index").to_numpy(zero_copy_only=False)
    score = flat.field("score").to_numpy(zero_copy_only=False)
    assert np.array_equal(index, np.array(pos, dtype=np.int64)[ei.astype(np.int64)][keep])
    assert np.array_equal(np.ascontiguousarray(score).view(np.uint64), es[keep].view(np.uint64))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("q,multiset", [(2, True), (3, False)])
def test_qgram_join_plugin_result_nulls_and_name(H, kind, q, multiset):
    X = F.near_duplicates()
    Q = [None if i % 7 == 3 else s for i, s in enumerate(X[:70])]
    Cs = [None if j % 5 == 1 else s for j, s in enumerate(X[40:90])] + ["Привет мир", "x" * 40] + list(X[:6])
    probe = {}
    got = H.call_plugin("qgram_join_" + kind, Q, Cs, names=("query", "cands"), _probe=probe, out_type=LIST, extra=mode(q, multiset) + [f64(0.7)])
    assert probe["name"] == "query" and probe["series_released"] == [1] * 5 and probe["arrays_released"] == [True] * 5
    _check(got, kind, q, multiset, Q, Cs, 0.7)
    assert got.null_count == sum(s is None for s in Q) and got.to_pylist()[3] is None
    # min_score absent, or null: every pair of the non-null rows
    _check(H.call_plugin("qgram_join_" + kind, Q, Cs, out_type=LIST, extra=mode(q, multiset)), kind, q, multiset, Q, Cs)
    _check(H.call_plugin("qgram_join_" + kind, Q, Cs, out_type=LIST, extra=mode(q, multiset) + [pa.array([None], type=pa.float64())]),
           kind, q, multiset, Q, Cs)


def test_qgram_join_plugin_small_columns(H):
    got = H.call_plugin("qgram_join_sorensen_dice", ["night", None, "abc"], ["nacht", "night", "cba"], out_type=LIST, extra=mode(2, True) + [f64(0.25)])
    assert got.to_pylist() == [[{"index": 0, "score": 0.25}, {"index": 1, "score": 1.0}], None, []]
    got = H.call_plugin("qgram_join_jaccard", ["abc"], ["cba", None], out_type=LIST, extra=mode(1, True) + [f64(1.0)])
    assert got.to_pylist() == [[{"index": 0, "score": 1.0}]]
    got = H.call_plugin("qgram_join_overlap", ["a", None], [None, None], out_type=LIST, extra=mode(2, False))
    assert got.to_pylist() == [[], None]
    got = H.call_plugin("qgram_join_cosine", pa.array([], type=pa.string()), ["a"], out_type=LIST, extra=mode(3, True))
    assert got.to_pylist() == [] and got.type == LIST
    got = H.call_plugin("qgram_join_cosine", ["ab", "abc"], ["ba", "ab"], out_type=LIST, extra=mode(2, True) + [f64(1.5)])
    assert got.to_pylist() == [[], []]


def test_qgram_join_plugin_shape_and_argument_errors(H):
    Q, Cs = ["abc", "abd"], ["abd", "xyz", "q"]
    bad = [
        ([], "qgram_join: expected 2 input series .*got 2"),
        ([u32(2)], "qgram_join: expected 2 input series .*got 3"),
        (mode(2, True) + [f64(0.5), f64(0.6)], "qgram_join: expected 2 input series .*got 6"),
        ([u32(0), u32(0)], "q=0 is outside 1..3"),
        ([u32(4), u32(0)], "q=4 is outside 1..3"),
        ([u32(2), u32(2)], "the set flag must be 0 or 1, got 2"),
        ([f64(2.0), u32(0)], "q must be a UInt32 series"),
        ([u32(2), f64(0.0)], "the set flag must be a UInt32 series"),
        ([pa.array([2, 3], type=pa.uint32()), u32(0)], "q must be a single value"),
        (mode(2, True) + [pa.array([0.5, 0.6], type=pa.float64())], "score_cutoff must be a single value"),
        (mode(2, True) + [f64(float("nan"))], "score_cutoff must not be NaN"),
        (mode(2, True) + [u32(1)], "score_cutoff must be a Float64"),
    ]
    for kind in KINDS:
        for extra, words in bad:
            with pytest.raises(H.PluginError, match=words):
                H.call_plugin("qgram_join_" + kind, Q, Cs, out_type=LIST, extra=extra)


@pytest.mark.parametrize("kind,q,multiset,cut", [("sorensen_dice", 2, True, 0.8), ("jaccard", 3, False, 0.7)])
def test_qgram_cluster_plugin_roots_nulls_name_and_type(H, kind, q, multiset, cut):
    full = F.cluster_column()
    col = [None if i % 7 == 5 else s for i, s in enumerate(full)]
    pos = [i for i, s in enumerate(col) if s is not None]
    kept = [col[i] for i in pos]
    found = R.join(kind, kept, kept, cut, q, multiset, True)
    root, _, count, nnz = cluster_ref.cluster(None, kept, cut, found=found)
    assert 0 < nnz and 1 < count < len(kept)
    exp = [None] * len(col)
    for x, r in zip(pos, root):
        exp[x] = pos[r]
    probe = {}
    got = H.call_plugin("qgram_cluster_" + kind, col, u32(q), names=("name", "q"), _probe=probe, out_type=U32,
                        extra=[u32(0 if multiset else 1), f64(cut)])
    assert probe["name"] == "name" and got.type == U32 and got.to_pylist() == exp and got.null_count == len(col) - len(pos)
    assert exp[0] == exp[1] == exp[2] == 0  # the chain


def test_qgram_cluster_plugin_small_columns_and_errors(H):
    got = H.call_plugin("qgram_cluster_sorensen_dice", ["night", None, "nights", "nacht", None, "night"], u32(2), out_type=U32, extra=[u32(0), f64(0.8)])
    assert got.to_pylist() == [0, None, 0, 3, None, 0]
    got = H.call_plugin("qgram_cluster_jaccard", [None, None], u32(2), out_type=U32, extra=[u32(1), f64(0.8)])
    assert got.to_pylist() == [None, None]
    got = H.call_plugin("qgram_cluster_cosine", pa.array([], type=pa.string()), u32(3), out_type=U32, extra=[u32(0), f64(0.8)])
    assert got.to_pylist() == []
    col = ["abc", "abd"]
    bad = [
        ((u32(2), []), "qgram_cluster: expected 4 input series .*got 2"),
        ((u32(2), [u32(0)]), "qgram_cluster: expected 4 input series .*got 3"),
        ((u32(2), [u32(0), f64(0.5), f64(0.5)]), "qgram_cluster: expected 4 input series .*got 5"),
        ((u32(5), [u32(0), f64(0.5)]), "q=5 is outside 1..3"),
        ((u32(2), [u32(3), f64(0.5)]), "the set flag must be 0 or 1, got 3"),
        ((u32(2), [u32(0), pa.array([None], type=pa.float64())]), "min_score must not be null"),
        ((u32(2), [u32(0), f64(float("nan"))]), "min_score must not be NaN"),
        ((u32(2), [u32(0), u32(1)]), "min_score must be a Float64 series"),
    ]
    for kind in KINDS:
        for (b, extra), words in bad:
            with pytest.raises(H.PluginError, match=words):
                H.call_plugin("qgram_cluster_" + kind, col, b, out_type=U32, extra=extra)
