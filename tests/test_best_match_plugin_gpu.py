"""The best_match_<measure> plugin functions end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host).  Expected values: the CPU oracle's scores, then the top-1 with the tie rule (tests/best_match_ref.py)."""
import numpy as np
import pyarrow as pa
import pytest

import best_match_ref as R
import gen

pytestmark = pytest.mark.gpu
MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")
STRUCT = pa.struct([pa.field("index", pa.uint32()), pa.field("score", pa.float64())])


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def expect(measure, Q, Cs):
    """list of {index, score} or None: nulls dropped from the candidates, indices of the caller's positions"""
    pos = [j for j, c in enumerate(Cs) if c is not None]
    sc = R.score_matrix(measure, [q if q is not None else "" for q in Q], [Cs[j] for j in pos])
    idx, val = R.topk(sc, 1)
    out = []
    for i, q in enumerate(Q):
        if q is None or idx[i, 0] < 0:
            out.append(None)
        else:
            out.append({"index": pos[idx[i, 0]], "score": float(val[i, 0])})
    return out


def check(got, exp):
    got = got.to_pylist()
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        if e is None:
            assert g is None, i
        else:
            assert g is not None and g["index"] == e["index"], (i, g, e)
            assert np.float64(g["score"]).view(np.uint64) == np.float64(e["score"]).view(np.uint64), (i, g, e)


@pytest.mark.parametrize("measure", MEASURES)
def test_struct_result_and_name(H, measure):
    Q = ["apple", "banana", "cherry", "", "kiwi"]
    Cs = ["banan", "appel", "chery", "kiwi", "apple"]
    probe = {}
    got = H.call_plugin("best_match_" + measure, Q, Cs, names=("query", "cands"), _probe=probe, out_type=STRUCT)
    assert got.type == STRUCT
    assert probe["name"] == "query"
    assert probe["series_released"] == [1, 1] and probe["arrays_released"] == [True, True]
    check(got, expect(measure, Q, Cs))


@pytest.mark.parametrize("measure", MEASURES)
def test_field_declares_the_struct(H, measure):
    name, typ = H.field_plugin("best_match_" + measure, ("query", "cands"))
    assert name == "query" and typ == STRUCT


@pytest.mark.parametrize("layout", ["vu", "u", ("u", "vu"), ("vu", "U")])
def test_nulls_multichunk_and_index_remap(H, layout):
    A, B = gen.pairs(77, 300, gen.ASCII_LOWER, 0, 20)
    Q = [None if i % 7 == 3 else a for i, a in enumerate(A)]
    Cs = [None if j % 5 == 1 else b for j, b in enumerate(B[:123])] + ["Привет", "x" * 40]
    qa = pa.chunked_array([pa.array(Q[:100]), pa.array(Q[100:101]), pa.array(Q[101:])])
    ca = pa.chunked_array([pa.array(Cs[:50]), pa.array(Cs[50:])])
    for m in ("levenshtein", "jaro_winkler"):
        got = H.call_plugin("best_match_" + m, qa, ca, layout=layout, out_type=STRUCT)
        check(got, expect(m, Q, Cs))


def test_all_candidates_null_or_none(H):
    got = H.call_plugin("best_match_jaro", ["a", None, "b"], [None, None], out_type=STRUCT)
    assert got.to_pylist() == [None, None, None]


def test_error_then_next_call_succeeds(H):
    with pytest.raises(H.PluginError, match="dtype"):
        H.call_plugin("best_match_levenshtein", pa.array([1, 2, 3]), ["a"], out_type=STRUCT)
    got = H.call_plugin("best_match_levenshtein", ["abc"], ["abd", "abc"], out_type=STRUCT)
    assert got.to_pylist() == [{"index": 1, "score": 1.0}]
