"""The cluster_<measure> plugin functions end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host).  Expected values: the roots of tests/cluster_ref.py over the non-null rows, mapped back to their rows of the
input; null for a null row."""
import functools

import pyarrow as pa
import pytest

import cluster_frames as F
import cluster_ref as R

pytestmark = pytest.mark.gpu
U32 = pa.uint32()


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def lit(v):
    return pa.array([v], type=pa.float64())


@functools.lru_cache(maxsize=None)
def model(measure):
    """(column with nulls, min_score, expected roots) -- computed once per measure"""
    full = F.frame(43)
    col = tuple(None if i % 7 == 3 else s for i, s in enumerate(full))
    cut = F.MIN_SCORE[measure]
    pos = [i for i, s in enumerate(col) if s is not None]
    kept = [col[i] for i in pos]
    found = R.hits(measure, kept, cut)
    assert R.worth_it(measure, kept, cut, found)  # on the model: clusters of several members that chain
    root = R.cluster(measure, kept, cut, found)[0]
    exp = [None] * len(col)
    for x, r in zip(pos, root):
        exp[x] = pos[r]
    return col, cut, exp


@pytest.mark.parametrize("measure", R.CLUSTER_MEASURES)
def test_cluster_plugin_roots_nulls_name_and_type(H, measure):
    col, cut, exp = model(measure)
    probe = {}
    got = H.call_plugin("cluster_" + measure, list(col), lit(cut), names=("name", "min_score"), _probe=probe, out_type=U32)
    assert probe["name"] == "name"
    assert probe["series_released"] == [1, 1] and probe["arrays_released"] == [True, True]
    assert got.type == U32 and got.num_chunks == 1 and len(got) == len(col)
    assert got.null_count == sum(s is None for s in col)
    assert got.to_pylist() == exp


@pytest.mark.parametrize("measure", ["jaro_winkler", "token_sort_ratio"])
@pytest.mark.parametrize("layout", ["vu", "u"])
def test_cluster_plugin_two_chunks_are_one_column(H, measure, layout):
    col, cut, exp = model(measure)
    two = pa.chunked_array([pa.array(list(col[:61])), pa.array(list(col[61:]))])
    got = H.call_plugin("cluster_" + measure, two, lit(cut), layout=(layout, "u"), out_type=U32)
    assert len(got) == len(col) and got.to_pylist() == exp
    assert any(r is not None and r < 61 <= i for i, r in enumerate(exp))  # a group spans the chunk boundary


def test_cluster_plugin_small_columns(H):
    got = H.call_plugin("cluster_ratio", ["anna", None, "ana", "bob", None, "anna"], lit(0.8), out_type=U32)
    assert got.to_pylist() == [0, None, 0, 3, None, 0]
    got = H.call_plugin("cluster_levenshtein", [None, None], lit(0.8), out_type=U32)
    assert got.to_pylist() == [None, None]
    got = H.call_plugin("cluster_jaro", pa.array([], type=pa.string()), lit(0.8), out_type=U32)
    assert got.to_pylist() == [] and got.type == U32
    got = H.call_plugin("cluster_jaccard", ["ab", "ab", "ba"], lit(1.5), out_type=U32)
    assert got.to_pylist() == [0, 1, 2]
    got = H.call_plugin("cluster_sorensen_dice", ["ab", "xy", "ba"], lit(float("-inf")), out_type=U32)
    assert got.to_pylist() == [0, 0, 0]


@pytest.mark.parametrize("measure", R.CLUSTER_MEASURES)
def test_cluster_plugin_errors(H, measure):
    probe = {}
    with pytest.raises(H.PluginError, match=r"cluster: expected 2 input series \(the column and the Float64 literal min_score\), got 1"):
        H.call_plugin_unary("cluster_" + measure, ["a", "b"], _probe=probe, out_type=U32)
    assert probe["series_released"] == [1] and probe["arrays_released"] == [True]
    bad = [
        (pa.array([0.5, 0.6], type=pa.float64()), "min_score must be a single value"),
        (pa.array([float("nan")], type=pa.float64()), "min_score must not be NaN"),
        (pa.array([None], type=pa.float64()), "min_score must not be null"),
        (pa.array([1], type=pa.int64()), "min_score must be a Float64"),
    ]
    for second, words in bad:
        with pytest.raises(H.PluginError, match=words):
            H.call_plugin("cluster_" + measure, ["a", "b"], second, out_type=U32)
    with pytest.raises(H.PluginError, match="invalid series dtype: expected `String`"):
        H.call_plugin("cluster_" + measure, pa.array([1, 2]), lit(0.5), out_type=U32)
