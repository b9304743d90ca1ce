"""The levenshtein_distance / osa_distance plugin functions end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host): nulls, chunked inputs, the "vu" and "u" layouts, a literal on either side, the max_distance input and its
errors, ShapeMismatch, and concurrent calls from several threads."""
import threading

import pyarrow as pa
import pytest

import distance_ref as R
import gen

pytestmark = pytest.mark.gpu
FUNCS = (("levenshtein_distance", "levenshtein"), ("osa_distance", "osa"))


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def cutoff(k):
    return [pa.array([k], type=pa.uint32())]


def expect(measure, A, B, k=None):
    n = max(len(A), len(B))
    A = A * n if len(A) == 1 else A
    B = B * n if len(B) == 1 else B
    return [None if (a is None or b is None) else R.distance(measure, a, b, k) for a, b in zip(A, B)]


def frame(seed, n):
    A, B = gen.pairs(seed, n, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(seed + 1, n // 5, gen.MIXED, 0, 90)
    A, B = A + A2 + ["ab" * 40], B + B2 + ["ba" * 40]
    for i in range(0, len(A), 37):
        A[i] = None
    for i in range(5, len(B), 41):
        B[i] = None
    return A, B


@pytest.mark.parametrize("fn,measure", FUNCS)
def test_dist_plugin_nulls_layouts_and_chunks(H, fn, measure):
    A, B = frame(21, 1500)
    want = expect(measure, A, B)
    for layout in ("vu", "u"):
        probe = {}
        got = H.call_plugin(fn, A, B, layout=layout, names=("left", "right"), out_type=pa.uint32(), _probe=probe)
        assert probe["name"] == "left" and got.type == pa.uint32()
        assert got.to_pylist() == want
    ca = pa.chunked_array([pa.array(A[:700]), pa.array(A[700:])])
    cb = pa.chunked_array([pa.array(B[:333]), pa.array(B[333:1200]), pa.array(B[1200:])])
    assert H.call_plugin(fn, ca, cb, out_type=pa.uint32()).to_pylist() == want


@pytest.mark.parametrize("fn,measure", FUNCS)
def test_dist_plugin_literal_either_side(H, fn, measure):
    A, _ = frame(22, 600)
    for lit in ("jonh", "héllo", ""):
        want = expect(measure, [lit], A)
        assert H.call_plugin(fn, [lit], A, out_type=pa.uint32()).to_pylist() == want
        assert H.call_plugin(fn, A, [lit], out_type=pa.uint32()).to_pylist() == want
    assert H.call_plugin(fn, A, [None], out_type=pa.uint32()).to_pylist() == [None] * len(A)


@pytest.mark.parametrize("fn,measure", FUNCS)
def test_dist_plugin_max_distance_input(H, fn, measure):
    A, B = frame(23, 1000)
    for k in (0, 1, 3, 0xFFFFFFFF):
        got = H.call_plugin(fn, A, B, out_type=pa.uint32(), extra=cutoff(k)).to_pylist()
        assert got == expect(measure, A, B, k), k


def test_dist_plugin_bad_max_distance(H):
    A, B = ["abc", "abd"], ["abd", "xyz"]
    bad = [
        ([pa.array([1, 2], type=pa.uint32())], "single value"),
        ([pa.array([], type=pa.uint32())], "single value"),
        ([pa.array([None], type=pa.uint32())], "must not be null"),
        ([pa.array([1], type=pa.int64())], "UInt32"),
        ([pa.array(["1"])], "UInt32"),
    ]
    for extra, words in bad:
        with pytest.raises(H.PluginError, match=words):
            H.call_plugin("levenshtein_distance", A, B, out_type=pa.uint32(), extra=extra)
    with pytest.raises(H.PluginError, match="expected 2 input series"):
        H.call_plugin("osa_distance", A, B, out_type=pa.uint32(), extra=cutoff(1) + cutoff(2))


def test_dist_plugin_shape_mismatch(H):
    with pytest.raises(H.PluginError, match="Inputs must have the same length, or one of them must be a Utf8 literal."):
        H.call_plugin("osa_distance", ["a", "b", "c"], ["a", "b"], out_type=pa.uint32())


def test_dist_plugin_concurrent_threads(H):
    A, B = frame(24, 800)
    want = {(m, k): expect(m, A, B, k) for _, m in FUNCS for k in (None, 2)}
    errors = []

    def worker(i):
        try:
            for j in range(6):
                fn, m = FUNCS[(i + j) % 2]
                k = None if j % 3 else 2
                got = H.call_plugin(fn, A, B, out_type=pa.uint32(), parallel=bool(i % 2),
                                    extra=() if k is None else cutoff(k)).to_pylist()
                if got != want[(m, k)]:
                    errors.append((i, j))
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
