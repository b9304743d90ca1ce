"""The nearest_levenshtein / nearest_osa plugin functions end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host).  Expected values: distance_ref's distances, then the top-1 with the tie rule (tests/nearest_ref.py)."""
import pyarrow as pa
import pytest

import gen
import nearest_ref as R

pytestmark = pytest.mark.gpu
MEASURES = ("levenshtein", "osa")
STRUCT = pa.struct([pa.field("index", pa.uint32()), pa.field("distance", pa.uint32())])


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def cutoff(k):
    return [pa.array([k], type=pa.uint32())]


def expect(measure, Q, Cs, md=None):
    """list of {index, distance} or None: nulls dropped from the candidates, indices of the caller's positions"""
    pos = [j for j, c in enumerate(Cs) if c is not None]
    dm = R.distance_matrix(measure, [q if q is not None else "" for q in Q], [Cs[j] for j in pos])
    idx, val = R.topk(dm, 1, md)
    return [None if q is None or idx[i, 0] < 0 else {"index": pos[idx[i, 0]], "distance": int(val[i, 0])} for i, q in enumerate(Q)]


@pytest.mark.parametrize("measure", MEASURES)
def test_nearest_plugin_struct_result_and_name(H, measure):
    Q = ["apple", "banana", "cherry", "", "kiwi", "ab"]
    Cs = ["banan", "appel", "chery", "kiwi", "apple", "ba"]
    probe = {}
    got = H.call_plugin("nearest_" + measure, Q, Cs, names=("query", "cands"), _probe=probe, out_type=STRUCT)
    assert got.type == STRUCT
    assert probe["name"] == "query"
    assert probe["series_released"] == [1, 1] and probe["arrays_released"] == [True, True]
    assert got.to_pylist() == expect(measure, Q, Cs)


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("layout", ["vu", "u", ("u", "vu")])
def test_nearest_plugin_nulls_both_sides_and_max_distance(H, measure, layout):
    A, B = gen.pairs(97, 300, gen.ASCII_LOWER, 0, 20)
    Q = [None if i % 7 == 3 else a for i, a in enumerate(A)]
    Cs = [None if j % 5 == 1 else b for j, b in enumerate(B[:123])] + ["Привет", "x" * 40]
    qa = pa.chunked_array([pa.array(Q[:100]), pa.array(Q[100:101]), pa.array(Q[101:])])
    ca = pa.chunked_array([pa.array(Cs[:50]), pa.array(Cs[50:])])
    got = H.call_plugin("nearest_" + measure, qa, ca, layout=layout, out_type=STRUCT)
    assert got.to_pylist() == expect(measure, Q, Cs)
    for md in (0, 2):
        got = H.call_plugin("nearest_" + measure, qa, ca, layout=layout, out_type=STRUCT, extra=cutoff(md))
        exp = expect(measure, Q, Cs, md)
        assert got.to_pylist() == exp
        assert any(e is None for e, q in zip(exp, Q) if q is not None)  # the cutoff leaves some queries without a match


def test_nearest_plugin_all_candidates_null(H):
    got = H.call_plugin("nearest_levenshtein", ["a", None, "b"], [None, None], out_type=STRUCT)
    assert got.to_pylist() == [None, None, None]


def test_nearest_plugin_bad_max_distance(H):
    Q, Cs = ["abc", "abd"], ["abd", "xyz", "q"]
    bad = [
        ([pa.array([1, 2], type=pa.uint32())], "single value"),
        ([pa.array([None], type=pa.uint32())], "must not be null"),
        ([pa.array([1], type=pa.int64())], "UInt32"),
    ]
    for extra, words in bad:
        with pytest.raises(H.PluginError, match=words):
            H.call_plugin("nearest_osa", Q, Cs, out_type=STRUCT, extra=extra)
    with pytest.raises(H.PluginError, match="expected 2 input series"):
        H.call_plugin("nearest_levenshtein", Q, Cs, out_type=STRUCT, extra=cutoff(1) + cutoff(2))
