"""The osa plugin function end to end on the GPU, with pyarrow standing in for the Polars engine (strsim_amd.arrow_host): nulls,
chunked and misaligned inputs, both engine modes, literal broadcast, the null literal, ShapeMismatch, and concurrent calls through
the combiner (its open batches are indexed by measure id)."""
import json
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

import gen
import osa_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "helpers", "osa_coalesce_child.py")


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def expect(A, B):
    n = max(len(A), len(B))
    A = A * n if len(A) == 1 else A
    B = B * n if len(B) == 1 else B
    return [None if (a is None or b is None) else R.score(a, b) for a, b in zip(A, B)]


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
    A, B = A + A2 + ["ab" * 300], B + B2 + ["ba" * 300]
    for i in range(0, len(A), 37):
        A[i] = None
    for i in range(5, len(B), 41):
        B[i] = None
    return A, B


def test_name_and_field(H):
    probe = {}
    got = H.call_plugin("osa", ["jonh", "martha"], ["john", "marhta"], names=("left", "right"), _probe=probe)
    assert probe["name"] == "left" and got.type == pa.float64()
    check(got, [0.75, 0.8333333333333334])
    assert H.field_plugin("osa", ("left", "right")) == ("left", pa.float64())


@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("layout", ["vu", "u"])
def test_nulls_chunks_and_slices(H, parallel, layout):
    A, B = frame(31, 6000)
    exp = expect(A, B)
    pa_a, pa_b = pa.array(A, pa.string()), pa.array(B, pa.string())
    ca = pa.chunked_array([pa_a[:7], pa_a[7:1000], pa_a[1000:1000], pa_a[1000:4999], pa_a[4999:]])
    cb = pa.chunked_array([pa_b[:2048], pa_b[2048:2049], pa_b[2049:]])
    check(H.call_plugin("osa", ca, cb, layout=layout, parallel=parallel), exp)
    big_a = pa.array(["pad"] * 3 + A + ["pad"] * 5, pa.string())[3:3 + len(A)]
    check(H.call_plugin("osa", big_a, pa_b, layout=layout, parallel=parallel), exp)


def test_literal_either_side_and_null_cases(H):
    A, _ = frame(40, 2000)
    for lit in ("phillips", "mülelr", "z" * 100):
        check(H.call_plugin("osa", A, lit), expect(A, [lit]))
        check(H.call_plugin("osa", lit, A), expect([lit], A))
    check(H.call_plugin("osa", A, [None]), [None] * len(A))
    check(H.call_plugin("osa", [None] * 10, [None] * 10), [None] * 10)
    check(H.call_plugin("osa", ["x"], ["x"]), [1.0])
    assert H.call_plugin("osa", [], []).to_pylist() == []


def test_shape_mismatch(H):
    with pytest.raises(H.PluginError, match="same length"):
        H.call_plugin("osa", ["a", "b"], ["a", "b", "c"])


def test_large_call_over_several_slices(H, monkeypatch):
    monkeypatch.setenv("POLARS_STRSIM_DIRECT_ROWS", "0")
    A, B = gen.pairs(50, 300_000, gen.ASCII_LOWER, 0, 24)
    A[1000] = "é" * 500
    B[1000] = "é" * 499 + "ü"
    A[7] = None
    short = [i for i in range(len(A)) if i != 1000]  # (batch_numpy pads every row to the longest one)
    exp = [None] * len(A)
    for i, v in zip(short, R.batch_numpy([A[i] or "" for i in short], [B[i] for i in short]).tolist()):
        exp[i] = v
    exp[1000] = R.score(A[1000], B[1000])
    exp[7] = None
    check(H.call_plugin("osa", A, B), exp)


def test_concurrent_calls_through_the_combiner():
    env = {k: v for k, v in os.environ.items() if not k.startswith("POLARS_STRSIM_")}
    env.update({"POLARS_STRSIM_COALESCE": "1", "POLARS_STRSIM_COALESCE_MIN_INFLIGHT": "1"})
    r = subprocess.run([sys.executable, CHILD, "4", "25"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["bad"] == [] and d["calls_combined"] >= 50
