"""The extract_ratio / extract_token_sort_ratio plugin functions end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host).  Expected values: the scores of tests/extract_ref.py, then the top-1 with the tie rule and the cutoff."""
import pyarrow as pa
import pytest

import extract_ref as R
import gen
import token_ref

pytestmark = pytest.mark.gpu
SCORERS = R.SCORERS
STRUCT = pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def cutoff(v):
    return [pa.array([v], type=pa.float64())]


def expect(scorer, Q, Cs, cut=None):
    """list of {index, score} or None: nulls dropped from the candidates, indices of the caller's positions"""
    pos = [j for j, c in enumerate(Cs) if c is not None]
    idx, val = R.extract(scorer, [q if q is not None else "" for q in Q], [Cs[j] for j in pos], 1, cut)
    return [None if q is None or idx[i, 0] < 0 else {"index": pos[idx[i, 0]], "score": float(val[i, 0])} for i, q in enumerate(Q)]


@pytest.mark.parametrize("scorer", SCORERS)
def test_extract_plugin_struct_result_and_name(H, scorer):
    Q = ["apple pie", "banana", "cherry", "", "kiwi", "ab", "pie  apple"]
    Cs = ["banan", "pie apple", "chery", "kiwi", "apple pie", "ba", "abxxxx"]
    probe = {}
    got = H.call_plugin("extract_" + scorer, Q, Cs, names=("query", "cands"), _probe=probe, out_type=STRUCT)
    assert got.type == STRUCT
    assert probe["name"] == "query"
    assert probe["series_released"] == [1, 1] and probe["arrays_released"] == [True, True]
    assert got.to_pylist() == expect(scorer, Q, Cs)
    if scorer == "token_sort_ratio":
        assert got.to_pylist()[0] == {"index": 1, "score": 1.0}  # the lower of the two candidates that normalise to "apple pie"


@pytest.mark.parametrize("scorer", SCORERS)
@pytest.mark.parametrize("layout", ["vu", "u", ("u", "vu")])
def test_extract_plugin_nulls_both_sides_and_score_cutoff(H, scorer, layout):
    if scorer == "ratio":
        A, B = gen.pairs(97, 300, gen.ASCII_LOWER, 0, 20)
    else:
        A, B = token_ref.gen_frame(97, 300)
    Q = [None if i % 7 == 3 else a for i, a in enumerate(A)]
    Cs = [None if j % 5 == 1 else b for j, b in enumerate(B[:123])] + ["Привет мир", "x" * 40]
    qa = pa.chunked_array([pa.array(Q[:100]), pa.array(Q[100:101]), pa.array(Q[101:])])
    ca = pa.chunked_array([pa.array(Cs[:50]), pa.array(Cs[50:])])
    got = H.call_plugin("extract_" + scorer, qa, ca, layout=layout, out_type=STRUCT)
    assert got.to_pylist() == expect(scorer, Q, Cs)
    # a null cutoff is no cutoff
    got = H.call_plugin("extract_" + scorer, qa, ca, layout=layout, out_type=STRUCT, extra=[pa.array([None], type=pa.float64())])
    assert got.to_pylist() == expect(scorer, Q, Cs)
    for cut in (0.0, 0.8, 1.0):
        got = H.call_plugin("extract_" + scorer, qa, ca, layout=layout, out_type=STRUCT, extra=cutoff(cut))
        exp = expect(scorer, Q, Cs, cut)
        assert got.to_pylist() == exp
        if cut > 0.0:  # the cutoff leaves some queries without a match: a null row
            assert any(e is None for e, q in zip(exp, Q) if q is not None)
            assert any(e is not None for e in exp)


def test_extract_plugin_all_candidates_null(H):
    got = H.call_plugin("extract_ratio", ["a", None, "b"], [None, None], out_type=STRUCT)
    assert got.to_pylist() == [None, None, None]
    got = H.call_plugin("extract_ratio", ["a", None, "b"], ["a"], out_type=STRUCT, extra=cutoff(1.5))
    assert got.to_pylist() == [None, None, None]


def test_extract_plugin_bad_score_cutoff(H):
    Q, Cs = ["abc", "abd"], ["abd", "xyz", "q"]
    bad = [
        ([pa.array([0.5, 0.6], type=pa.float64())], "score_cutoff must be a single value"),
        ([pa.array([float("nan")], type=pa.float64())], "score_cutoff must not be NaN"),
        ([pa.array([1], type=pa.int64())], "score_cutoff must be a Float64"),
        ([pa.array([1], type=pa.uint32())], "score_cutoff must be a Float64"),
    ]
    for fn in ("extract_ratio", "extract_token_sort_ratio"):
        for extra, words in bad:
            with pytest.raises(H.PluginError, match=words):
                H.call_plugin(fn, Q, Cs, out_type=STRUCT, extra=extra)
        with pytest.raises(H.PluginError, match="expected 2 input series"):
            H.call_plugin(fn, Q, Cs, out_type=STRUCT, extra=cutoff(0.5) + cutoff(0.6))
