"""The distance_join_<kind> and distance_cluster_<kind> plugin functions end to end on the GPU, with pyarrow standing in for the
Polars engine (strsim_amd.arrow_host).  Expected values: the hits of tests/distance_join_ref.py over the non-null candidates, mapped
back to their rows of input 1, a null list for a null query; the roots of tests/cluster_ref.py over the non-null rows, null for a
null row."""
import numpy as np
import pyarrow as pa
import pytest

import cluster_ref
import distance_join_frames as F
import distance_join_ref as R

pytestmark = pytest.mark.gpu
KINDS = R.MEASURES
LIST = pa.large_list(pa.field("item", pa.struct([pa.field("index", pa.uint32()), pa.field("distance", pa.uint32())])))
U32 = pa.uint32()


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def u32(v):
    return pa.array([v], type=pa.uint32())


def _check(got, kind, Q, Cs, k=None):
    """the one chunk of a result against the model: offsets, list validity, indices and distances"""
    n = len(Q)
    assert got.type == LIST and got.num_chunks == 1 and len(got) == n
    arr = got.chunk(0)
    pos = [j for j, c in enumerate(Cs) if c is not None]
    ep, ei, ed = R.join(kind, [s if s is not None else "" for s in Q], [Cs[j] for j in pos], k)
    valid = np.array([s is not None for s in Q], dtype=bool)
    counts = np.where(valid, np.diff(ep.astype(np.int64)), 0)
    assert 0 < counts.sum() < valid.sum() * len(pos) or k is None
    assert arr.offsets.to_pylist() == [0] + np.cumsum(counts).tolist()
    assert np.asarray(arr.is_valid()).tolist() == valid.tolist()
    keep = np.repeat(valid, np.diff(ep.astype(np.int64)))
    flat = arr.values
    assert flat.null_count == 0 and len(flat) == int(keep.sum())
    index = flat.field("index").to_numpy(zero_copy_only=False)
    dist = flat.field("distance").to_numpy(zero_copy_only=False)
    assert np.array_equal(index, np.array(pos, dtype=np.int64)[ei.astype(np.int64)][keep])
    assert np.array_equal(dist, ed[keep])


@pytest.mark.parametrize("kind", KINDS)
def test_distance_join_plugin_result_nulls_and_name(H, kind):
    X = F.near_duplicates()
    Q = [None if i % 7 == 3 else s for i, s in enumerate(X[:70])]
    Cs = [None if j % 5 == 1 else s for j, s in enumerate(X[40:90])] + ["Привет мир", "x" * 40] + list(X[:6])
    probe = {}
    got = H.call_plugin("distance_join_" + kind, Q, Cs, names=("query", "cands"), _probe=probe, out_type=LIST, extra=[u32(2)])
    assert probe["name"] == "query" and probe["series_released"] == [1] * 3 and probe["arrays_released"] == [True] * 3
    _check(got, kind, Q, Cs, 2)
    assert got.null_count == sum(s is None for s in Q) and got.to_pylist()[3] is None
    # max_distance absent, or null: every pair of the non-null rows
    _check(H.call_plugin("distance_join_" + kind, Q, Cs, out_type=LIST), kind, Q, Cs)
    _check(H.call_plugin("distance_join_" + kind, Q, Cs, out_type=LIST, extra=[pa.array([None], type=pa.uint32())]), kind, Q, Cs)
    _check(H.call_plugin("distance_join_" + kind, Q, Cs, out_type=LIST, extra=[u32(0)]), kind, Q, Cs, 0)


def test_distance_join_plugin_small_columns(H):
    got = H.call_plugin("distance_join_levenshtein", ["night", None, "abc"], ["nacht", "night", "cba"], out_type=LIST, extra=[u32(2)])
    assert got.to_pylist() == [[{"index": 0, "distance": 2}, {"index": 1, "distance": 0}], None, [{"index": 2, "distance": 2}]]
    got = H.call_plugin("distance_join_damerau_levenshtein", ["ca"], ["abc", None, "ac"], out_type=LIST, extra=[u32(2)])
    assert got.to_pylist() == [[{"index": 0, "distance": 2}, {"index": 2, "distance": 1}]]
    got = H.call_plugin("distance_join_osa", ["ca"], ["abc", None, "ac"], out_type=LIST, extra=[u32(2)])
    assert got.to_pylist() == [[{"index": 2, "distance": 1}]]
    got = H.call_plugin("distance_join_osa", ["a", None], [None, None], out_type=LIST, extra=[u32(1)])
    assert got.to_pylist() == [[], None]
    got = H.call_plugin("distance_join_osa", pa.array([], type=pa.string()), ["a"], out_type=LIST)
    assert got.to_pylist() == [] and got.type == LIST
    got = H.call_plugin("distance_join_levenshtein", ["ab", "abc"], ["xy", "q"], out_type=LIST, extra=[u32(1)])
    assert got.to_pylist() == [[], []]


def test_distance_join_plugin_shape_and_argument_errors(H):
    Q, Cs = ["abc", "abd"], ["abd", "xyz", "q"]
    bad = [
        ([u32(1), u32(1)], "distance_join: expected 2 input series .*got 4"),
        ([pa.array([2.0], type=pa.float64())], "max_distance must be a UInt32 series"),
        ([pa.array([1, 2], type=pa.uint32())], "max_distance must be a single value"),
        ([pa.array([], type=pa.uint32())], "max_distance must be a single value, got 0 rows"),
    ]
    for kind in KINDS:
        for extra, words in bad:
            with pytest.raises(H.PluginError, match=words):
                H.call_plugin("distance_join_" + kind, Q, Cs, out_type=LIST, extra=extra)


@pytest.mark.parametrize("kind,k", [("levenshtein", 2), ("damerau_levenshtein", 2), ("osa", 1)])
def test_distance_cluster_plugin_roots_nulls_name_and_type(H, kind, k):
    full = F.cluster_column()[:150]
    col = [None if i % 7 == 5 else s for i, s in enumerate(full)]
    pos = [i for i, s in enumerate(col) if s is not None]
    kept = [col[i] for i in pos]
    found = R.join(kind, kept, kept, k, True)
    root, _, count, nnz = cluster_ref.cluster(None, kept, k, found=found)
    assert 0 < nnz and 1 < count < len(kept)
    exp = [None] * len(col)
    for x, r in zip(pos, root):
        exp[x] = pos[r]
    probe = {}
    got = H.call_plugin("distance_cluster_" + kind, col, u32(k), names=("name", "k"), _probe=probe, out_type=U32)
    assert probe["name"] == "name" and got.type == U32 and got.to_pylist() == exp and got.null_count == len(col) - len(pos)
    if k == 2:
        assert exp[0] == exp[1] == exp[2] == 0  # the chain


def test_distance_cluster_plugin_small_columns_and_errors(H):
    got = H.call_plugin("distance_cluster_osa", ["night", None, "nigth", "nacht", None, "night"], u32(1), out_type=U32)
    assert got.to_pylist() == [0, None, 0, 3, None, 0]
    got = H.call_plugin("distance_cluster_levenshtein", ["night", None, "nigth", "nacht", None, "night"], u32(1), out_type=U32)
    assert got.to_pylist() == [0, None, 2, 3, None, 0]
    got = H.call_plugin("distance_cluster_osa", [None, None], u32(2), out_type=U32)
    assert got.to_pylist() == [None, None]
    got = H.call_plugin("distance_cluster_damerau_levenshtein", pa.array([], type=pa.string()), u32(3), out_type=U32)
    assert got.to_pylist() == []
    col = ["abc", "abd"]
    bad = [
        ((u32(2), [u32(0)]), "distance_cluster: expected 2 input series .*got 3"),
        ((pa.array([None], type=pa.uint32()), []), "max_distance must not be null"),
        ((pa.array([0.5]), []), "max_distance must be a UInt32 series"),
        ((pa.array([1, 2], type=pa.uint32()), []), "max_distance must be a single value"),
    ]
    for kind in KINDS:
        for (b, extra), words in bad:
            with pytest.raises(H.PluginError, match=words):
                H.call_plugin("distance_cluster_" + kind, col, b, out_type=U32, extra=extra)
