"""The token_sort_ratio / token_set_ratio plugin functions end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host): nulls, chunked and sliced inputs, the "vu" and "u" layouts, both engine modes, literal broadcast, the null
literal, ShapeMismatch, a 100 000-row call through the sliced pipeline and concurrent calls from eight threads."""
import threading

import numpy as np
import pyarrow as pa
import pytest

import indel_ref
import token_ref as R

pytestmark = pytest.mark.gpu
FUNCTIONS = ("token_sort_ratio", "token_set_ratio")


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


@pytest.fixture(scope="module")
def cref():
    return indel_ref.CRef()


def expect(fn, A, B, cref):
    """The model's scores, None under a null of either side."""
    A, B = R.broadcast(list(A), list(B))
    f = R.token_sort_ratio if fn == "token_sort_ratio" else R.set_rule
    return [None if a is None or b is None else f(a, b, cref.lcs) for a, b in zip(A, B)]


def check(got, exp):
    got = got.to_pylist()
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        if e is None:
            assert g is None, i
        else:
            assert g is not None and np.float64(g).view(np.uint64) == np.float64(e).view(np.uint64), (i, g, e)


def frame(seed, n):
    A, B = R.gen_frame(seed, n)
    A += ["café au lait", "漢字 漢 字", "w" * 70 + " v", " ".join("t%d" % i for i in range(20)), "", "  ", "a\u3000b\u00a0c"]
    B += ["lait café", "字 漢字", "v " + "w" * 70, " ".join("t%d" % i for i in range(19, -1, -1)), " ", "x", "c b a"]
    for i in range(0, len(A), 37):
        A[i] = None
    for i in range(5, len(B), 41):
        B[i] = None
    return A, B


def test_names_types_and_fields(H):
    probe = {}
    for fn, exp in (("token_sort_ratio", [1.0, 0.5]), ("token_set_ratio", [1.0, 1.0])):
        got = H.call_plugin(fn, ["smith john", "a a"], ["john  smith", "a"], names=("left", "right"), _probe=probe)
        assert probe["name"] == "left" and got.type == pa.float64()
        check(got, exp)
        assert H.field_plugin(fn, ("left", "right")) == ("left", pa.float64())


@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("layout", ["vu", "u"])
def test_nulls_chunks_and_slices(H, cref, fn, parallel, layout):
    A, B = frame(31, 6000)
    scores = expect(fn, A, B, cref)
    pa_a, pa_b = pa.array(A, pa.string()), pa.array(B, pa.string())
    ca = pa.chunked_array([pa_a[:7], pa_a[7:1000], pa_a[1000:1000], pa_a[1000:4999], pa_a[4999:]])
    cb = pa.chunked_array([pa_b[:2048], pa_b[2048:2049], pa_b[2049:]])
    check(H.call_plugin(fn, ca, cb, layout=layout, parallel=parallel), scores)
    big_a = pa.array(["pad"] * 3 + A + ["pad"] * 5, pa.string())[3:3 + len(A)]
    check(H.call_plugin(fn, big_a, pa_b, layout=layout, parallel=parallel), scores)


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_literal_either_side_and_null_cases(H, cref, fn):
    A, _ = frame(40, 2000)
    for lit in ("smith john", "déjà vu", "z" * 100 + " y", "", " "):
        check(H.call_plugin(fn, A, lit), expect(fn, A, [lit], cref))
        check(H.call_plugin(fn, lit, A), expect(fn, [lit], A, cref))
    check(H.call_plugin(fn, A, [None]), [None] * len(A))
    check(H.call_plugin(fn, [None] * 10, [None] * 10), [None] * 10)
    check(H.call_plugin(fn, ["x y"], ["y x"]), [1.0])
    assert H.call_plugin(fn, [], []).to_pylist() == []
    with pytest.raises(H.PluginError, match="same length"):
        H.call_plugin(fn, ["a", "b"], ["a", "b", "c"])


@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("parallel", [False, True])
def test_100k_rows_in_both_engine_modes(H, fn, parallel, monkeypatch):
    monkeypatch.setenv("POLARS_STRSIM_DIRECT_ROWS", "0")
    A, B = R.gen_frame(50, 100_000)
    exp = (R.frame_sort_ratio if fn == "token_sort_ratio" else R.frame_set_ratio)(A, B)
    exp = [float(x) for x in exp]
    A[1000], B[1000] = "é" * 500 + " a", "a " + "é" * 499 + "ü"
    exp[1000] = (R.token_sort_ratio if fn == "token_sort_ratio" else R.set_rule)(A[1000], B[1000])
    A[7] = None
    exp[7] = None
    check(H.call_plugin(fn, A, B, parallel=parallel), exp)


def test_eight_threads_calling_concurrently(H, cref):
    A, B = frame(24, 800)
    scores = {fn: expect(fn, A, B, cref) for fn in FUNCTIONS}
    errors = []

    def same(got, exp):
        got = got.to_pylist()
        return len(got) == len(exp) and all(
            (g is None) == (e is None) and (e is None or np.float64(g).view(np.uint64) == np.float64(e).view(np.uint64))
            for g, e in zip(got, exp))

    def worker(i):
        try:
            for j in range(6):
                fn = FUNCTIONS[(i + j) % 2]
                if not same(H.call_plugin(fn, A, B, parallel=bool(i % 2)), scores[fn]):
                    errors.append((i, j, fn))
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
