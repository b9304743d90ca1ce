"""The indel / indel_distance plugin functions end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host): nulls, chunked and sliced inputs, the "vu" and "u" layouts, both engine modes, literal broadcast, the null
literal, the max_distance input, ShapeMismatch, a 100 000-row call and concurrent calls from eight threads."""
import threading

import numpy as np
import pyarrow as pa
import pytest

import gen
import indel_ref as R

pytestmark = pytest.mark.gpu
U = R.UNBOUNDED


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
    return (A * n if len(A) == 1 and n != 1 else A), (B * n if len(B) == 1 and n != 1 else B)


def expect(A, B, cref):
    """-> (scores, distances), None under a null of either side."""
    A, B = bcast(A, B)
    live = [i for i in range(len(A)) if A[i] is not None and B[i] is not None]
    d = R.mixed_distances([A[i] for i in live], [B[i] for i in live], cref, short=32)
    s = R.scores_from_distances(d, [len(A[i]) for i in live], [len(B[i]) for i in live])
    scores, dists = [None] * len(A), [None] * len(A)
    for j, i in enumerate(live):
        scores[i], dists[i] = float(s[j]), int(d[j])
    return scores, dists


def clamp(dists, k):
    return [None if d is None else R.clamp(d, k) for d in dists]


def check(got, exp):
    got = got.to_pylist()
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        if e is None:
            assert g is None, i
        else:
            assert g is not None and np.float64(g).view(np.uint64) == np.float64(e).view(np.uint64), (i, g, e)


def frame(seed, n):
    A, B = gen.pairs(seed, n, gen.ASCII_LOWER, 0, 32)
    A2, B2 = gen.pairs(seed + 1, n // 10, gen.MIXED, 0, 90)
    A3, B3 = gen.pairs(seed + 2, n // 10, gen.ASCII_LOWER, 60, 128)
    A, B = A + A2 + A3 + ["ab" * 300], B + B2 + B3 + ["ba" * 300]
    for i in range(0, len(A), 37):
        A[i] = None
    for i in range(5, len(B), 41):
        B[i] = None
    return A, B


def test_names_types_and_fields(H):
    probe = {}
    got = H.call_plugin("indel", ["jonh", "ab"], ["john", "ba"], names=("left", "right"), _probe=probe)
    assert probe["name"] == "left" and got.type == pa.float64()
    check(got, [0.75, 0.5])
    got = H.call_plugin("indel_distance", ["jonh", "kitten"], ["john", "sitting"], names=("left", "right"), out_type=pa.uint32(), _probe=probe)
    assert probe["name"] == "left" and got.type == pa.uint32() and got.to_pylist() == [2, 5]
    assert H.field_plugin("indel", ("left", "right")) == ("left", pa.float64())
    assert H.field_plugin("indel_distance", ("left", "right", "max_distance")) == ("left", pa.uint32())


@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("layout", ["vu", "u"])
def test_nulls_chunks_and_slices(H, cref, parallel, layout):
    A, B = frame(31, 6000)
    scores, dists = expect(A, B, cref)
    pa_a, pa_b = pa.array(A, pa.string()), pa.array(B, pa.string())
    ca = pa.chunked_array([pa_a[:7], pa_a[7:1000], pa_a[1000:1000], pa_a[1000:4999], pa_a[4999:]])
    cb = pa.chunked_array([pa_b[:2048], pa_b[2048:2049], pa_b[2049:]])
    check(H.call_plugin("indel", ca, cb, layout=layout, parallel=parallel), scores)
    assert H.call_plugin("indel_distance", ca, cb, layout=layout, parallel=parallel, out_type=pa.uint32()).to_pylist() == dists
    big_a = pa.array(["pad"] * 3 + A + ["pad"] * 5, pa.string())[3:3 + len(A)]
    check(H.call_plugin("indel", big_a, pa_b, layout=layout, parallel=parallel), scores)
    assert H.call_plugin("indel_distance", big_a, pa_b, layout=layout, parallel=parallel, out_type=pa.uint32(),
                         extra=cutoff(3)).to_pylist() == clamp(dists, 3)


def test_literal_either_side_and_null_cases(H, cref):
    A, _ = frame(40, 2000)
    for lit in ("phillips", "mülelr", "z" * 100, "z" * 129, ""):
        scores, dists = expect(A, [lit], cref)
        check(H.call_plugin("indel", A, lit), scores)
        check(H.call_plugin("indel", lit, A), scores)
        assert H.call_plugin("indel_distance", A, [lit], out_type=pa.uint32()).to_pylist() == dists
        assert H.call_plugin("indel_distance", [lit], A, out_type=pa.uint32(), extra=cutoff(4)).to_pylist() == clamp(dists, 4)
    check(H.call_plugin("indel", A, [None]), [None] * len(A))
    assert H.call_plugin("indel_distance", A, [None], out_type=pa.uint32()).to_pylist() == [None] * len(A)
    check(H.call_plugin("indel", [None] * 10, [None] * 10), [None] * 10)
    check(H.call_plugin("indel", ["x"], ["x"]), [1.0])
    assert H.call_plugin("indel", [], []).to_pylist() == []
    assert H.call_plugin("indel_distance", [], [], out_type=pa.uint32()).to_pylist() == []


@pytest.mark.parametrize("k", [0, 1, 3, 16, U])
def test_max_distance_input(H, cref, k):
    A, B = frame(23, 1500)
    _, dists = expect(A, B, cref)
    assert H.call_plugin("indel_distance", A, B, out_type=pa.uint32(), extra=cutoff(k)).to_pylist() == clamp(dists, k)
    if k == U:
        assert H.call_plugin("indel_distance", A, B, out_type=pa.uint32()).to_pylist() == dists


def test_errors(H):
    with pytest.raises(H.PluginError, match="same length"):
        H.call_plugin("indel", ["a", "b"], ["a", "b", "c"])
    with pytest.raises(H.PluginError, match="same length"):
        H.call_plugin("indel_distance", ["a", "b"], ["a", "b", "c"], out_type=pa.uint32())
    with pytest.raises(H.PluginError, match="max_distance"):
        H.call_plugin("indel_distance", ["a"], ["b"], out_type=pa.uint32(), extra=[pa.array([1, 2], type=pa.uint32())])


@pytest.mark.parametrize("parallel", [False, True])
def test_100k_rows_in_both_engine_modes(H, cref, parallel, monkeypatch):
    monkeypatch.setenv("POLARS_STRSIM_DIRECT_ROWS", "0")
    A, B = gen.pairs(50, 100_000, gen.ASCII_LOWER, 0, 24)
    A[1000] = "é" * 500
    B[1000] = "é" * 499 + "ü"
    A[2000] = "ab" * 64
    B[2000] = "ba" * 64
    A[7] = None
    scores, dists = expect(A, B, cref)
    check(H.call_plugin("indel", A, B, parallel=parallel), scores)
    assert H.call_plugin("indel_distance", A, B, parallel=parallel, out_type=pa.uint32(), extra=cutoff(5)).to_pylist() == clamp(dists, 5)


def test_eight_threads_calling_concurrently(H, cref):
    A, B = frame(24, 800)
    scores, dists = expect(A, B, cref)
    errors = []

    def same(got):
        got = got.to_pylist()
        return len(got) == len(scores) and all(
            (g is None) == (e is None) and (e is None or np.float64(g).view(np.uint64) == np.float64(e).view(np.uint64))
            for g, e in zip(got, scores))

    def worker(i):
        try:
            for j in range(6):
                if (i + j) % 2:
                    if not same(H.call_plugin("indel", A, B, parallel=bool(i % 2))):
                        errors.append((i, j, "indel"))
                else:
                    k = None if j % 3 else 2
                    got = H.call_plugin("indel_distance", A, B, out_type=pa.uint32(), parallel=bool(i % 2),
                                        extra=() if k is None else cutoff(k)).to_pylist()
                    if got != (dists if k is None else clamp(dists, k)):
                        errors.append((i, j, "indel_distance"))
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
