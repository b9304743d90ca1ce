"""The token_ratio, partial_token_sort_ratio, partial_token_set_ratio, partial_token_ratio and wratio plugin functions end to end on
the GPU, with pyarrow standing in for the Polars engine (strsim_amd.arrow_host): the main frame of tests/wratio_frames.py with
nulls, chunked and sliced inputs, the "vu" and "u" layouts, both engine modes and the sliced pipeline, literal broadcast, the null
literal, ShapeMismatch, and concurrent calls from four threads."""
import threading

import numpy as np
import pyarrow as pa
import pytest

import wratio_frames as F
import wratio_ref as W

pytestmark = pytest.mark.gpu
FUNCTIONS = ("token_ratio", "partial_token_sort_ratio", "partial_token_set_ratio", "partial_token_ratio", "wratio")


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def with_nulls(A, B, scores):
    """Every 37th row of a and every 41st of b (from 5) null; the scores None under them."""
    A, B, exp = list(A), list(B), [float(x) for x in scores]
    for i in range(0, len(A), 37):
        A[i] = None
    for i in range(5, len(B), 41):
        B[i] = None
    return A, B, [None if a is None or b is None else e for a, b, e in zip(A, B, exp)]


def check(got, exp):
    got = got.to_pylist()
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        if e is None:
            assert g is None, i
        else:
            assert g is not None and np.float64(g).view(np.uint64) == np.float64(e).view(np.uint64), (i, g, e)


def test_wratio_plugin_names_types_and_fields(H):
    probe = {}
    a, b = ["this is a test", "ab ab"], ["this is a new test!!!", "abab"]
    for fn in FUNCTIONS:
        got = H.call_plugin(fn, a, b, names=("left", "right"), _probe=probe)
        assert probe["name"] == "left" and got.type == pa.float64()
        check(got, [W.SCORE[fn](x, y) for x, y in zip(a, b)])
        assert H.field_plugin(fn, ("left", "right")) == ("left", pa.float64())
    check(H.call_plugin("wratio", a, b), [(1.0 * 0.95) * 0.9, W.wratio("ab ab", "abab")])


@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("parallel,layout,direct", [(False, "vu", None), (True, "u", None), (False, "u", "0")])
def test_wratio_plugin_main_frame_nulls_chunks_and_slices(H, fn, parallel, layout, direct, monkeypatch):
    if direct is not None:
        monkeypatch.setenv("POLARS_STRSIM_DIRECT_ROWS", direct)  # the sliced pipeline instead of one direct call
    A0, B0, cols = F.main()
    A, B, scores = with_nulls(A0, B0, cols[fn])
    pa_a, pa_b = pa.array(A, pa.string()), pa.array(B, pa.string())
    ca = pa.chunked_array([pa_a[:7], pa_a[7:1000], pa_a[1000:1000], pa_a[1000:4999], pa_a[4999:]])
    cb = pa.chunked_array([pa_b[:2048], pa_b[2048:2049], pa_b[2049:]])
    check(H.call_plugin(fn, ca, cb, layout=layout, parallel=parallel), scores)
    if direct is None and not parallel:
        big_a = pa.array(["pad"] * 3 + A + ["pad"] * 5, pa.string())[3:3 + len(A)]
        check(H.call_plugin(fn, big_a, pa_b, layout=layout, parallel=parallel), scores)


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_wratio_plugin_literal_either_side_and_null_cases(H, fn):
    A, _, _ = F.take(F.mixed(250, seed=13))
    A += ["", "  ", "日本 ab", None]
    fr = F.frames()
    for lit in ("ab cd", "déjà vu", "", " "):
        X = ["" if s is None else s for s in A]
        e1, e2 = fr.columns(X, [lit])[fn], fr.columns([lit], X)[fn]
        check(H.call_plugin(fn, A, lit), [None if s is None else float(e) for s, e in zip(A, e1)])
        check(H.call_plugin(fn, lit, A), [None if s is None else float(e) for s, e in zip(A, e2)])
    check(H.call_plugin(fn, A, [None]), [None] * len(A))
    check(H.call_plugin(fn, [None] * 10, [None] * 10), [None] * 10)
    assert H.call_plugin(fn, [], []).to_pylist() == []
    with pytest.raises(H.PluginError, match="same length"):
        H.call_plugin(fn, ["a", "b"], ["a", "b", "c"])


def test_wratio_plugin_four_threads_calling_concurrently(H):
    A, B, cols = F.take(F.mixed(600, seed=17))
    frames = {fn: with_nulls(A, B, cols[fn]) for fn in FUNCTIONS}
    errors = []

    def same(got, exp):
        got = got.to_pylist()
        return len(got) == len(exp) and all(
            (g is None) == (e is None) and (e is None or np.float64(g).view(np.uint64) == np.float64(e).view(np.uint64))
            for g, e in zip(got, exp))

    def worker(i):
        try:
            for j in range(5):
                fn = FUNCTIONS[(i + j) % len(FUNCTIONS)]
                a, b, exp = frames[fn]
                if not same(H.call_plugin(fn, a, b, parallel=bool(i % 2)), exp):
                    errors.append((i, j, fn))
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
