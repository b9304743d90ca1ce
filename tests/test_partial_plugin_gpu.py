"""The partial_ratio / partial_ratio_alignment plugin functions end to end on the GPU, with pyarrow standing in for the Polars
engine (strsim_amd.arrow_host): field names and dtypes, nulls, chunked and sliced inputs, both string layouts, both engine modes,
literal broadcast, the null literal, ShapeMismatch.  The field functions run without a GPU."""
import numpy as np
import pyarrow as pa
import pytest

import gen
import partial_ref as R

STRUCT = pa.struct([("score", pa.float64()), ("src_start", pa.uint32()), ("src_end", pa.uint32()), ("dest_start", pa.uint32()),
                    ("dest_end", pa.uint32())])


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


@pytest.fixture(scope="module")
def cref():
    return R.CRef()


def bcast(A, B):
    n = max(len(A), len(B))
    return (A * n if len(A) == 1 and n != 1 else A), (B * n if len(B) == 1 and n != 1 else B)


def expect(A, B, cref):
    """-> one (score, src_start, src_end, dest_start, dest_end) per row, None under a null of either side."""
    A, B = bcast(A, B)
    live = [i for i in range(len(A)) if A[i] is not None and B[i] is not None]
    s, sp, _, _ = cref.batch([A[i] for i in live], [B[i] for i in live])
    out = [None] * len(A)
    for j, i in enumerate(live):
        out[i] = (float(s[j]),) + tuple(int(x) for x in sp[j])
    return out


def check_scores(got, exp):
    got = got.to_pylist()
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        if e is None:
            assert g is None, i
        else:
            assert g is not None and np.float64(g).view(np.uint64) == np.float64(e[0]).view(np.uint64), (i, g, e)


def check_structs(got, exp):
    assert got.type == STRUCT
    got = got.to_pylist()
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        if e is None:
            assert g is None, i
        else:
            assert g is not None, i
            assert np.float64(g["score"]).view(np.uint64) == np.float64(e[0]).view(np.uint64), (i, g, e)
            assert (g["src_start"], g["src_end"], g["dest_start"], g["dest_end"]) == e[1:], (i, g, e)


def frame(seed, n):
    A, B = gen.pairs(seed, n, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(seed + 1, n // 10, gen.MIXED, 0, 70)
    A3, B3 = gen.pairs(seed + 2, n // 10, "ab", 1, 32, p_edit=0.0, p_same=0.0)
    A, B = A + A2 + A3 + ["acme corp"], B + B2 + B3 + ["invoice 4411 - acme corp. ltd, rotterdam"]
    for i in range(0, len(A), 37):
        A[i] = None
    for i in range(5, len(B), 41):
        B[i] = None
    return A, B


def test_partial_plugin_field_functions(H):
    assert H.field_plugin("partial_ratio", ("left", "right")) == ("left", pa.float64())
    assert H.field_plugin("partial_ratio_alignment", ("left", "right")) == ("left", STRUCT)


@pytest.mark.gpu
def test_partial_plugin_names_and_types(H):
    probe = {}
    got = H.call_plugin("partial_ratio", ["jonh", "abcd"], ["mr john smith", "XXabcdXX"], names=("left", "right"), _probe=probe)
    assert probe["name"] == "left" and got.type == pa.float64() and got.to_pylist() == [0.75, 1.0]
    got = H.call_plugin("partial_ratio_alignment", ["jonh", "XXabcdXX"], ["mr john smith", "abcd"], names=("left", "right"),
                        out_type=STRUCT, _probe=probe)
    assert probe["name"] == "left" and got.type == STRUCT
    assert got.to_pylist() == [{"score": 0.75, "src_start": 0, "src_end": 4, "dest_start": 2, "dest_end": 6},
                               {"score": 1.0, "src_start": 2, "src_end": 6, "dest_start": 0, "dest_end": 4}]


@pytest.mark.gpu
@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("layout", ["vu", "u"])
def test_partial_plugin_nulls_chunks_and_slices(H, cref, parallel, layout):
    A, B = frame(61, 5000)
    exp = expect(A, B, cref)
    pa_a, pa_b = pa.array(A, pa.string()), pa.array(B, pa.string())
    ca = pa.chunked_array([pa_a[:7], pa_a[7:1000], pa_a[1000:1000], pa_a[1000:4999], pa_a[4999:]])
    cb = pa.chunked_array([pa_b[:2048], pa_b[2048:2049], pa_b[2049:]])
    check_scores(H.call_plugin("partial_ratio", ca, cb, layout=layout, parallel=parallel), exp)
    check_structs(H.call_plugin("partial_ratio_alignment", ca, cb, layout=layout, parallel=parallel, out_type=STRUCT), exp)
    big_a = pa.array(["pad"] * 3 + A + ["pad"] * 5, pa.string())[3:3 + len(A)]
    check_scores(H.call_plugin("partial_ratio", big_a, pa_b, layout=layout, parallel=parallel), exp)
    check_structs(H.call_plugin("partial_ratio_alignment", big_a, pa_b, layout=layout, parallel=parallel, out_type=STRUCT), exp)


@pytest.mark.gpu
def test_partial_plugin_literal_either_side_and_null_cases(H, cref):
    A, _ = frame(70, 2000)
    for lit in ("jonathan", "mülelr", "z" * 33, "acme corp ltd of rotterdam, the netherlands", ""):
        exp = expect(A, [lit], cref)
        check_scores(H.call_plugin("partial_ratio", A, lit), exp)
        check_structs(H.call_plugin("partial_ratio_alignment", A, [lit], out_type=STRUCT), exp)
        exp = expect([lit], A, cref)
        check_scores(H.call_plugin("partial_ratio", lit, A), exp)
        check_structs(H.call_plugin("partial_ratio_alignment", [lit], A, out_type=STRUCT), exp)
    check_scores(H.call_plugin("partial_ratio", A, [None]), [None] * len(A))
    check_structs(H.call_plugin("partial_ratio_alignment", A, [None], out_type=STRUCT), [None] * len(A))
    check_structs(H.call_plugin("partial_ratio_alignment", [None] * 10, [None] * 10, out_type=STRUCT), [None] * 10)
    check_structs(H.call_plugin("partial_ratio_alignment", ["x"], ["x"], out_type=STRUCT), [(1.0, 0, 1, 0, 1)])
    assert H.call_plugin("partial_ratio", [], []).to_pylist() == []
    assert H.call_plugin("partial_ratio_alignment", [], [], out_type=STRUCT).to_pylist() == []


@pytest.mark.gpu
def test_partial_plugin_errors(H):
    with pytest.raises(H.PluginError, match="same length"):
        H.call_plugin("partial_ratio", ["a", "b"], ["a", "b", "c"])
    with pytest.raises(H.PluginError, match="same length"):
        H.call_plugin("partial_ratio_alignment", ["a", "b"], ["a", "b", "c"], out_type=STRUCT)


@pytest.mark.gpu
def test_partial_plugin_50k_rows_through_the_pipeline(H, cref, monkeypatch):
    monkeypatch.setenv("POLARS_STRSIM_DIRECT_ROWS", "0")
    A, B = gen.pairs(80, 50_000, gen.ASCII_LOWER, 0, 24)
    A[1000] = "é" * 200
    B[1000] = "é" * 99 + "ü"
    A[7] = None
    exp = expect(A, B, cref)
    check_scores(H.call_plugin("partial_ratio", A, B, parallel=True), exp)
    check_structs(H.call_plugin("partial_ratio_alignment", A, B, out_type=STRUCT), exp)
