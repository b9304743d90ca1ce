"""The twelve hamming / prefix / postfix / lcs_seq plugin functions end to end on the GPU, with pyarrow standing in for the Polars
engine (strsim_amd.arrow_host): the output's name and dtype and the field callbacks, nulls on either side and in the literal, chunked
inputs and both string layouts, a literal on either side, the max_distance input present, absent and wrong, a third input to the
functions that take none, ShapeMismatch; results equal tests/common_ref.py."""
import numpy as np
import pyarrow as pa
import pytest

import common_ref as R
import gen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def cutoff(k):
    return [pa.array([k], type=pa.uint32())]


def bcast(A, B):
    n = max(len(A), len(B))
    return (A * n if len(A) == 1 else A), (B * n if len(B) == 1 else B)


def expect(kind, what, A, B, k=None):
    A, B = bcast(A, B)
    f = {"count": R.count, "distance": lambda kd, a, b: R.clamp(R.distance(kd, a, b), k), "score": R.score}[what]
    return [None if (a is None or b is None) else f(kind, a, b) for a, b in zip(A, B)]


def same_f64(got, want):
    got = got.to_pylist()
    assert [g is None for g in got] == [w is None for w in want]
    g = np.array([x for x in got if x is not None], dtype=np.float64).view(np.uint64)
    w = np.array([x for x in want if x is not None], dtype=np.float64).view(np.uint64)
    return np.array_equal(g, w)


def frame(seed, n):
    A, B = gen.pairs(seed, n, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(seed + 1, n // 5, gen.MIXED, 0, 90)
    A, B = A + A2 + ["ab" * 40, "prefix", "testing", ""], B + B2 + ["ab" * 39 + "ba", "preface", "running", ""]
    for i in range(0, len(A), 37):
        A[i] = None
    for i in range(5, len(B), 41):
        B[i] = None
    return A, B


@pytest.mark.parametrize("kind", R.KINDS)
def test_common_plugin_names_dtypes_nulls_layouts_and_chunks(H, kind):
    A, B = frame(21, 600)
    want_s, want_d, want_c = expect(kind, "score", A, B), expect(kind, "distance", A, B), expect(kind, "count", A, B)
    assert H.field_plugin(kind, ("left", "right")) == ("left", pa.float64())
    assert H.field_plugin(kind + "_distance", ("left", "right", "max_distance")) == ("left", pa.uint32())
    assert H.field_plugin(kind + "_similarity", ("left", "right")) == ("left", pa.uint32())
    for layout in ("vu", "u"):
        probe = {}
        got = H.call_plugin(kind, A, B, layout=layout, names=("left", "right"), _probe=probe)
        assert probe["name"] == "left" and got.type == pa.float64() and same_f64(got, want_s)
        probe = {}
        got = H.call_plugin(kind + "_distance", A, B, layout=layout, names=("left", "right"), out_type=pa.uint32(), _probe=probe)
        assert probe["name"] == "left" and got.type == pa.uint32() and got.to_pylist() == want_d
        probe = {}
        got = H.call_plugin(kind + "_similarity", A, B, layout=layout, names=("left", "right"), out_type=pa.uint32(), _probe=probe)
        assert probe["name"] == "left" and got.type == pa.uint32() and got.to_pylist() == want_c
    ca = pa.chunked_array([pa.array(A[:300]), pa.array(A[300:])])
    cb = pa.chunked_array([pa.array(B[:133]), pa.array(B[133:500]), pa.array(B[500:])])
    assert same_f64(H.call_plugin(kind, ca, cb), want_s)
    assert H.call_plugin(kind + "_distance", ca, cb, out_type=pa.uint32()).to_pylist() == want_d
    assert H.call_plugin(kind + "_similarity", ca, cb, out_type=pa.uint32()).to_pylist() == want_c


@pytest.mark.parametrize("kind", R.KINDS)
def test_common_plugin_literal_either_side(H, kind):
    A, _ = frame(22, 300)
    for lit in ("jonh", "héllo", "", "the quick brown fox jumps over the lazy dog"):
        for X, Y in (([lit], A), (A, [lit])):
            assert same_f64(H.call_plugin(kind, X, Y), expect(kind, "score", X, Y))
            assert H.call_plugin(kind + "_distance", X, Y, out_type=pa.uint32(), extra=cutoff(3)).to_pylist() == expect(kind, "distance", X, Y, 3)
            assert H.call_plugin(kind + "_similarity", X, Y, out_type=pa.uint32()).to_pylist() == expect(kind, "count", X, Y)
    for fn, t in ((kind, None), (kind + "_distance", pa.uint32()), (kind + "_similarity", pa.uint32())):
        assert H.call_plugin(fn, A, [None], out_type=t).to_pylist() == [None] * len(A)
        assert H.call_plugin(fn, [None], A, out_type=t).to_pylist() == [None] * len(A)


@pytest.mark.parametrize("kind", R.KINDS)
def test_common_plugin_max_distance_input(H, kind):
    A, B = frame(23, 500)
    for k in (0, 1, 3, 40, 0xFFFFFFFF):
        got = H.call_plugin(kind + "_distance", A, B, out_type=pa.uint32(), extra=cutoff(k)).to_pylist()
        assert got == expect(kind, "distance", A, B, k), k


def test_common_plugin_bad_inputs(H):
    A, B = ["abc", "abd"], ["abd", "xyz"]
    bad = [
        ([pa.array([1, 2], type=pa.uint32())], "single value"),
        ([pa.array([], type=pa.uint32())], "single value"),
        ([pa.array([None], type=pa.uint32())], "must not be null"),
        ([pa.array([1], type=pa.int64())], "UInt32"),
        ([pa.array(["1"])], "UInt32"),
    ]
    for kind in R.KINDS:
        for extra, words in bad:
            with pytest.raises(H.PluginError, match=words):
                H.call_plugin(kind + "_distance", A, B, out_type=pa.uint32(), extra=extra)
        with pytest.raises(H.PluginError, match="expected 2 input series"):
            H.call_plugin(kind + "_distance", A, B, out_type=pa.uint32(), extra=cutoff(1) + cutoff(2))
        # the count and the normalised form take no cutoff
        with pytest.raises(H.PluginError, match="expected 2 input series, got 3"):
            H.call_plugin(kind + "_similarity", A, B, out_type=pa.uint32(), extra=cutoff(1))
        with pytest.raises(H.PluginError, match="expected 2 input series, got 3"):
            H.call_plugin(kind, A, B, extra=cutoff(1))
        for fn, t in ((kind, None), (kind + "_distance", pa.uint32()), (kind + "_similarity", pa.uint32())):
            with pytest.raises(H.PluginError, match="Inputs must have the same length, or one of them must be a Utf8 literal."):
                H.call_plugin(fn, ["a", "b", "c"], ["a", "b"], out_type=t)
            assert H.call_plugin(fn, [], [], out_type=t).to_pylist() == []
