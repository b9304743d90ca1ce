"""The cdist_<measure> plugin functions end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host).  Expected values: the matrix of tests/cdist_ref.py with the cutoff rule, null lists for null queries and
null elements for null candidates.  Scores are compared bit for bit."""
import numpy as np
import pyarrow as pa
import pytest

import cdist_ref as R
import gen
import token_ref

pytestmark = pytest.mark.gpu
MEASURES = R.MEASURES
LIST = pa.large_list(pa.field("item", pa.float64()))


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def cutoff(v):
    return [pa.array([v], type=pa.float64())]


def _matrix(got, n, m):
    """the one chunk of a result -> (scores f64 [n, m], list validity [n], element validity [n, m])"""
    assert got.type == LIST and got.num_chunks == 1 and len(got) == n
    arr = got.chunk(0)
    assert arr.offsets.to_pylist() == [i * m for i in range(n + 1)]
    flat = arr.values
    assert len(flat) == n * m
    valid = np.asarray(flat.is_valid())
    vals = flat.fill_null(0.0).to_numpy(zero_copy_only=False) if flat.null_count else flat.to_numpy(zero_copy_only=False)
    return vals.reshape(n, m), np.asarray(arr.is_valid()), valid.reshape(n, m)


def _check(got, measure, Q, Cs, cut=None):
    n, m = len(Q), len(Cs)
    vals, lists, elems = _matrix(got, n, m)
    exp = R.cdist(measure, [q if q is not None else "" for q in Q], [c if c is not None else "" for c in Cs], cut)
    assert lists.tolist() == [q is not None for q in Q]
    assert (elems == np.array([c is not None for c in Cs], dtype=bool)[None, :]).all()
    keep = lists[:, None] & elems
    assert np.array_equal(vals.view(np.uint64)[keep], exp.view(np.uint64)[keep])


@pytest.mark.parametrize("measure", MEASURES)
def test_cdist_plugin_list_result_and_name(H, measure):
    if measure == "token_sort_ratio":
        A, B = token_ref.gen_frame(171, 70)
    else:
        A, B = gen.pairs(171, 70, gen.ASCII_LOWER, 0, 14)
    Q, Cs = A, B[:40]
    probe = {}
    got = H.call_plugin("cdist_" + measure, Q, Cs, names=("query", "cands"), _probe=probe, out_type=LIST)
    assert probe["name"] == "query"
    assert probe["series_released"] == [1, 1] and probe["arrays_released"] == [True, True]
    _check(got, measure, Q, Cs)
    assert got.null_count == 0 and got.chunk(0).values.null_count == 0
    row = got.to_pylist()[3]
    assert len(row) == 40 and row == R.score_matrix(measure, [Q[3]], Cs)[0].tolist()


@pytest.mark.parametrize("measure", ["jaro_winkler", "ratio", "token_sort_ratio"])
@pytest.mark.parametrize("layout", ["vu", "u", ("u", "vu")])
def test_cdist_plugin_nulls_both_sides_and_score_cutoff(H, measure, layout):
    A, B = token_ref.gen_frame(173, 120) if measure == "token_sort_ratio" else gen.pairs(173, 120, gen.ASCII_LOWER, 0, 20)
    Q = [None if i % 7 == 3 else a for i, a in enumerate(A)]
    Cs = [None if j % 5 == 1 else b for j, b in enumerate(B[:43])] + ["Привет мир", "x" * 40]
    qa = pa.chunked_array([pa.array(Q[:50]), pa.array(Q[50:51]), pa.array(Q[51:])])
    ca = pa.chunked_array([pa.array(Cs[:20]), pa.array(Cs[20:])])
    got = H.call_plugin("cdist_" + measure, qa, ca, layout=layout, out_type=LIST)
    _check(got, measure, Q, Cs)
    assert got.null_count == sum(q is None for q in Q)
    assert got.chunk(0).values.null_count == len(Q) * sum(c is None for c in Cs)
    rows = got.to_pylist()
    assert rows[3] is None and rows[0][1] is None and rows[0][0] is not None
    # a null cutoff is no cutoff
    _check(H.call_plugin("cdist_" + measure, qa, ca, layout=layout, out_type=LIST, extra=[pa.array([None], type=pa.float64())]), measure, Q, Cs)
    for cut in (0.0, 0.6, 1.0, 1.5):
        _check(H.call_plugin("cdist_" + measure, qa, ca, layout=layout, out_type=LIST, extra=cutoff(cut)), measure, Q, Cs, cut)


def test_cdist_plugin_empty_sides_and_all_candidates_null(H):
    got = H.call_plugin("cdist_ratio", ["a", None, "b"], [None, None], out_type=LIST)
    assert got.to_pylist() == [[None, None], None, [None, None]]
    got = H.call_plugin("cdist_ratio", ["a", None], pa.array([], type=pa.string()), out_type=LIST)
    assert got.to_pylist() == [[], None]
    got = H.call_plugin("cdist_jaro", pa.array([], type=pa.string()), ["a"], out_type=LIST)
    assert got.to_pylist() == []
    got = H.call_plugin("cdist_ratio", ["ab", "abc"], ["ba"], out_type=LIST, extra=cutoff(1.5))
    assert got.to_pylist() == [[0.0], [0.0]]
    got = H.call_plugin("cdist_ratio", ["ab", "abc"], ["ba"], out_type=LIST, extra=cutoff(0.5))
    assert got.to_pylist() == [[0.5], [0.0]]


def test_cdist_plugin_bad_score_cutoff(H):
    Q, Cs = ["abc", "abd"], ["abd", "xyz", "q"]
    bad = [
        ([pa.array([0.5, 0.6], type=pa.float64())], "score_cutoff must be a single value"),
        ([pa.array([float("nan")], type=pa.float64())], "score_cutoff must not be NaN"),
        ([pa.array([1], type=pa.int64())], "score_cutoff must be a Float64"),
        ([pa.array([1], type=pa.uint32())], "score_cutoff must be a Float64"),
    ]
    for fn in ("cdist_ratio", "cdist_levenshtein", "cdist_token_sort_ratio"):
        for extra, words in bad:
            with pytest.raises(H.PluginError, match=words):
                H.call_plugin(fn, Q, Cs, out_type=LIST, extra=extra)
        with pytest.raises(H.PluginError, match="cdist: expected 2 input series"):
            H.call_plugin(fn, Q, Cs, out_type=LIST, extra=cutoff(0.5) + cutoff(0.6))


def test_cdist_plugin_frame_larger_than_one_slice(H):
    # 2 100 x 2 100 doubles are 35 MB: two slices of the 32 MB staging.  Against the matrix of one Context.cdist call (itself
    # tested against the model), and sampled rows against the model
    import strsim_amd as S
    A, B = gen.pairs(175, 2100, gen.ASCII_LOWER, 0, 12)
    A[1999] = None
    got = H.call_plugin("cdist_levenshtein", A, B, out_type=LIST)
    vals, lists, elems = _matrix(got, 2100, 2100)
    assert elems.all() and lists.sum() == 2099 and not lists[1999]
    with S.Context(0) as ctx:
        whole = ctx.cdist("levenshtein", *S.pack_strings([a or "" for a in A]), *S.pack_strings(B))
    assert np.array_equal(vals.view(np.uint64)[lists], whole.view(np.uint64)[lists])
    rows = [0, 1023, 1998, 2000, 2099]  # either side of the slice boundary at row 1 997
    exp = R.score_matrix("levenshtein", [A[i] for i in rows], B)
    assert np.array_equal(vals[rows].view(np.uint64), exp.view(np.uint64))
