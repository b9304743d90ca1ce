"""The qgram_jaccard / qgram_sorensen_dice / qgram_overlap / qgram_cosine plugin functions end to end on the GPU, with pyarrow
standing in for the Polars engine (strsim_amd.arrow_host): nulls on either side and in the literal, chunked inputs and both string
layouts, the q and set-flag inputs and their errors, ShapeMismatch, and the output's name and dtype."""
import numpy as np
import pyarrow as pa
import pytest

import gen
import qgram_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def u32(v):
    return pa.array([v], type=pa.uint32())


def expect(kind, A, B, q, multiset):
    n = max(len(A), len(B))
    A = A * n if len(A) == 1 else A
    B = B * n if len(B) == 1 else B
    return [None if (a is None or b is None) else R.score(kind, a, b, q, multiset) for a, b in zip(A, B)]


def same(got, want):
    got = got.to_pylist()
    assert [g is None for g in got] == [w is None for w in want]
    g = np.array([x for x in got if x is not None], dtype=np.float64).view(np.uint64)
    w = np.array([x for x in want if x is not None], dtype=np.float64).view(np.uint64)
    return np.array_equal(g, w)


def frame(seed, n):
    A, B = gen.pairs(seed, n, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(seed + 1, n // 5, gen.MIXED, 0, 90)
    A, B = A + A2 + ["ab" * 40, "a", ""], B + B2 + ["ba" * 40, "a", ""]
    for i in range(0, len(A), 37):
        A[i] = None
    for i in range(5, len(B), 41):
        B[i] = None
    return A, B


@pytest.mark.parametrize("kind", R.KINDS)
def test_qgram_plugin_nulls_layouts_chunks_name_and_dtype(H, kind):
    A, B = frame(21, 1000)
    want = expect(kind, A, B, 2, True)
    for layout in ("vu", "u"):
        probe = {}
        got = H.call_plugin("qgram_" + kind, A, B, layout=layout, names=("left", "right"), extra=[u32(2)], _probe=probe)
        assert probe["name"] == "left" and got.type == pa.float64()
        assert probe["series_released"] == [1, 1, 1]
        assert same(got, want)
    ca = pa.chunked_array([pa.array(A[:700]), pa.array(A[700:])])
    cb = pa.chunked_array([pa.array(B[:333]), pa.array(B[333:900]), pa.array(B[900:])])
    assert same(H.call_plugin("qgram_" + kind, ca, cb, extra=[u32(2), u32(0)]), want)
    assert H.field_plugin("qgram_" + kind, ("left", "right", "q")) == ("left", pa.float64())


@pytest.mark.parametrize("q,multiset", [(1, True), (2, False), (3, True), (3, False)])
def test_qgram_plugin_q_and_set_flag(H, q, multiset):
    A, B = frame(23, 600)
    for kind in ("jaccard", "cosine"):
        got = H.call_plugin("qgram_" + kind, A, B, extra=[u32(q), u32(0 if multiset else 1)])
        assert same(got, expect(kind, A, B, q, multiset)), (kind, q, multiset)


def test_qgram_plugin_literal_either_side_and_null_literal(H):
    A, _ = frame(22, 500)
    for lit in ("night", "héllo", "", "a", "ab" * 40):
        want = expect("sorensen_dice", [lit], A, 2, True)
        assert same(H.call_plugin("qgram_sorensen_dice", [lit], A, extra=[u32(2)]), want)
        assert same(H.call_plugin("qgram_sorensen_dice", A, [lit], extra=[u32(2)]), want)
    assert H.call_plugin("qgram_overlap", A, [None], extra=[u32(3), u32(1)]).to_pylist() == [None] * len(A)
    assert H.call_plugin("qgram_overlap", [None], A, extra=[u32(3)]).to_pylist() == [None] * len(A)
    assert H.call_plugin("qgram_cosine", [], [], extra=[u32(2)]).to_pylist() == []


def test_qgram_plugin_shape_error(H):
    with pytest.raises(H.PluginError, match="Inputs must have the same length, or one of them must be a Utf8 literal."):
        H.call_plugin("qgram_jaccard", ["a", "b"], ["a", "b", "c"], extra=[u32(2)])


def test_qgram_plugin_missing_or_bad_q(H):
    A, B = ["abc", "abd"], ["abd", "xyz"]
    with pytest.raises(H.PluginError, match="q is missing"):
        H.call_plugin("qgram_jaccard", A, B)
    bad = [
        ([pa.array([1, 2], type=pa.uint32())], "q must be a single value, got 2 rows"),
        ([pa.array([], type=pa.uint32())], "q must be a single value, got 0 rows"),
        ([pa.array([None], type=pa.uint32())], "q must not be null"),
        ([pa.array([2], type=pa.int64())], "q must be a UInt32 series, got Arrow format 'l'"),
        ([pa.array([2.0], type=pa.float64())], "q must be a UInt32 series"),
        ([u32(0)], "q=0 is outside 1..3"),
        ([u32(4)], "q=4 is outside 1..3"),
        ([u32(2), u32(2)], "the set flag must be 0 or 1, got 2"),
        ([u32(2), pa.array([None], type=pa.uint32())], "the set flag must not be null"),
        ([u32(2), pa.array([True], type=pa.bool_())], "the set flag must be a UInt32 series"),
        ([u32(2), u32(0), u32(0)], "expected 2 input series, q and an optional set flag, got 5 inputs"),
    ]
    for extra, msg in bad:
        for fn in ("qgram_jaccard", "qgram_cosine"):
            with pytest.raises(H.PluginError, match=msg):
                H.call_plugin(fn, A, B, extra=extra)
    # and the call after a refused one is served
    assert same(H.call_plugin("qgram_jaccard", A, B, extra=[u32(2)]), expect("jaccard", A, B, 2, True))
