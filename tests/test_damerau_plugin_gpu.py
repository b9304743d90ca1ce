"""The damerau_levenshtein / damerau_levenshtein_distance plugin functions end to end on the GPU, with pyarrow standing in for the
Polars engine (strsim_amd.arrow_host): the output's name and dtype, nulls on either side and in the literal, chunked inputs and both
string layouts, the max_distance input present, absent, null and of the wrong dtype, ShapeMismatch; results equal the C ABI's."""
import numpy as np
import pyarrow as pa
import pytest

import damerau_ref as R
import gen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


@pytest.fixture(scope="module")
def cref():
    return R.CRef()


def cutoff(k):
    return [pa.array([k], type=pa.uint32())]


def bcast(A, B):
    n = max(len(A), len(B))
    return (A * n if len(A) == 1 else A), (B * n if len(B) == 1 else B)


def expect_distance(cref, A, B, k=None):
    A, B = bcast(A, B)
    return [None if (a is None or b is None) else int(R.clamp([cref.distance(a, b)], k)[0]) for a, b in zip(A, B)]


def expect_score(cref, A, B):
    A, B = bcast(A, B)
    return [None if (a is None or b is None) else cref.score(a, b) for a, b in zip(A, B)]


def same(got, want):
    got = got.to_pylist()
    assert [g is None for g in got] == [w is None for w in want]
    g = np.array([x for x in got if x is not None], dtype=np.float64).view(np.uint64)
    w = np.array([x for x in want if x is not None], dtype=np.float64).view(np.uint64)
    return np.array_equal(g, w)


def frame(seed, n):
    A, B = gen.pairs(seed, n, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(seed + 1, n // 5, gen.MIXED, 0, 90)
    A, B = A + A2 + ["ab" * 40, "ca", ""], B + B2 + ["ba" * 40, "abc", ""]
    for i in range(0, len(A), 37):
        A[i] = None
    for i in range(5, len(B), 41):
        B[i] = None
    return A, B


def test_dl_plugin_similarity_nulls_layouts_chunks_name_and_dtype(H, cref):
    A, B = frame(21, 1000)
    want = expect_score(cref, A, B)
    for layout in ("vu", "u"):
        probe = {}
        got = H.call_plugin("damerau_levenshtein", A, B, layout=layout, names=("left", "right"), _probe=probe)
        assert probe["name"] == "left" and got.type == pa.float64()
        assert probe["series_released"] == [1, 1]
        assert same(got, want)
    ca = pa.chunked_array([pa.array(A[:700]), pa.array(A[700:])])
    cb = pa.chunked_array([pa.array(B[:333]), pa.array(B[333:900]), pa.array(B[900:])])
    assert same(H.call_plugin("damerau_levenshtein", ca, cb), want)
    assert H.field_plugin("damerau_levenshtein", ("left", "right")) == ("left", pa.float64())
    with pytest.raises(H.PluginError, match="expected 2 input series, got 3"):
        H.call_plugin("damerau_levenshtein", A, B, extra=cutoff(1))


def test_dl_plugin_distance_nulls_layouts_chunks_name_and_dtype(H, cref):
    A, B = frame(22, 1000)
    want = expect_distance(cref, A, B)
    for layout in ("vu", "u"):
        probe = {}
        got = H.call_plugin("damerau_levenshtein_distance", A, B, layout=layout, names=("left", "right"), out_type=pa.uint32(), _probe=probe)
        assert probe["name"] == "left" and got.type == pa.uint32()
        assert got.to_pylist() == want
    ca = pa.chunked_array([pa.array(A[:700]), pa.array(A[700:])])
    cb = pa.chunked_array([pa.array(B[:333]), pa.array(B[333:900]), pa.array(B[900:])])
    assert H.call_plugin("damerau_levenshtein_distance", ca, cb, out_type=pa.uint32()).to_pylist() == want
    assert H.field_plugin("damerau_levenshtein_distance", ("l", "r", "max_distance")) == ("l", pa.uint32())


def test_dl_plugin_literal_either_side_and_null_literal(H, cref):
    A, _ = frame(23, 500)
    for lit in ("jonh", "héllo", "", "ab" * 40):
        want = expect_score(cref, [lit], A)
        assert same(H.call_plugin("damerau_levenshtein", [lit], A), want)
        assert same(H.call_plugin("damerau_levenshtein", A, [lit]), want)
        want = expect_distance(cref, [lit], A, 4)
        assert H.call_plugin("damerau_levenshtein_distance", [lit], A, out_type=pa.uint32(), extra=cutoff(4)).to_pylist() == want
        assert H.call_plugin("damerau_levenshtein_distance", A, [lit], out_type=pa.uint32(), extra=cutoff(4)).to_pylist() == want
    assert H.call_plugin("damerau_levenshtein", A, [None]).to_pylist() == [None] * len(A)
    assert H.call_plugin("damerau_levenshtein_distance", [None], A, out_type=pa.uint32()).to_pylist() == [None] * len(A)
    assert H.call_plugin("damerau_levenshtein", [], []).to_pylist() == []
    assert H.call_plugin("damerau_levenshtein_distance", [], [], out_type=pa.uint32()).to_pylist() == []


def test_dl_plugin_max_distance_input(H, cref):
    A, B = frame(24, 800)
    for k in (0, 1, 3, 0xFFFFFFFF):
        got = H.call_plugin("damerau_levenshtein_distance", A, B, out_type=pa.uint32(), extra=cutoff(k)).to_pylist()
        assert got == expect_distance(cref, A, B, None if k == 0xFFFFFFFF else k), k


def test_dl_plugin_bad_max_distance_and_shape(H, cref):
    A, B = ["abc", "ca"], ["abd", "abc"]
    bad = [
        ([pa.array([1, 2], type=pa.uint32())], "single value"),
        ([pa.array([], type=pa.uint32())], "single value"),
        ([pa.array([None], type=pa.uint32())], "must not be null"),
        ([pa.array([1], type=pa.int64())], "UInt32"),
        ([pa.array(["1"])], "UInt32"),
    ]
    for extra, words in bad:
        with pytest.raises(H.PluginError, match=words):
            H.call_plugin("damerau_levenshtein_distance", A, B, out_type=pa.uint32(), extra=extra)
    with pytest.raises(H.PluginError, match="expected 2 input series"):
        H.call_plugin("damerau_levenshtein_distance", A, B, out_type=pa.uint32(), extra=cutoff(1) + cutoff(2))
    for fn, kw in (("damerau_levenshtein", {}), ("damerau_levenshtein_distance", {"out_type": pa.uint32()})):
        with pytest.raises(H.PluginError, match="Inputs must have the same length, or one of them must be a Utf8 literal."):
            H.call_plugin(fn, ["a", "b", "c"], ["a", "b"], **kw)
    # and the call after a refused one is served
    assert H.call_plugin("damerau_levenshtein_distance", A, B, out_type=pa.uint32()).to_pylist() == [1, 2]


def test_dl_plugin_equals_the_c_abi(H):
    import strsim_amd as S
    A, B = gen.pairs(25, 1200, gen.MIXED, 0, 70)
    with S.Context(0) as c:
        sim = c.damerau_host(*S.pack_strings(A), *S.pack_strings(B))
        d2 = c.damerau_distance_host(*S.pack_strings(A), *S.pack_strings(B), 2)
    got = np.array(H.call_plugin("damerau_levenshtein", A, B).to_pylist(), dtype=np.float64)
    assert np.array_equal(got.view(np.uint64), sim.view(np.uint64))
    assert H.call_plugin("damerau_levenshtein_distance", A, B, out_type=pa.uint32(), extra=cutoff(2)).to_pylist() == d2.tolist()
