"""The ONE JSON line of bench.py (the driver's contract): every required key, the two extra objects (roofline, cpu_baseline), the fields
added in round 6 and the arithmetic that ties them together -- on a small frame, so that it runs in seconds."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENV = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=_ENV, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line"
    return json.loads(lines[0])


def test_the_line_carries_the_contract_and_adds_up():
    d = _bench("--rows", "4000000", "--steps", "6", "--warmup", "2")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    # value = rows x steps / time
    assert abs(d["value"] - 4_000_000 / d["ms_per_step"] / 1e3) / d["value"] < 1e-6
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert abs(r["achieved"] - r["algorithmic_read_bytes"] / (r["kernel_ms"] * 1e-3) / 1e9) / r["achieved"] < 1e-6
    assert r["kernel_ms"] <= d["ms_per_step"] * 1.02  # the kernel fits inside the step
    # the counters are never taken inside a bench run: a replayed figure names its source, a missing one says so
    assert isinstance(r["traffic_source"], str) and (r["traffic"] is None) == r["traffic_source"].startswith("none")
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "rows" in c["sample"]
    assert d["parity_vs_oracle_on_sample"]["bit_mismatches"] == 0
    # round 6: the default call mode beside the headline's, one cold call, one call on an idle GPU, the mode read back from the context
    assert d["config"]["call_mode"].startswith("one_launch") and d["config"]["enqueued_kernels_and_copies_per_step"] == 1.0
    assert d["value_default_mode"] > 0 and d["default_mode"]["enqueued_kernels_and_copies_per_step"] == 5.0
    assert d["default_mode"]["call_mode"].startswith("stream_ordered")
    assert d["cold_first_call_ms"] > d["idle_gpu_call_ms"] > 0


def test_extra_modes_can_be_switched_off():
    d = _bench("--rows", "1000000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-e2e", "--no-extra-modes")
    assert d["value_default_mode"] is None and d["cold_first_call_ms"] is None and d["idle_gpu_call_ms"] is None and "cpu_baseline" not in d


def test_dump_outputs_holds_what_the_timed_steps_computed(tmp_path):
    """--dump-outputs: the last timed step's column, bit for bit the oracle's on the same synthetic rows -- every row of a small frame,
    a seeded sample within 64 MB of a large one, the same sample in every run."""
    import numpy as np
    import oracle_lib as O
    from bench_support import workload as W
    _, _, law, lo, hi, seed = W.CONFIGS["cfg2"]
    quiet = ("--no-cpu-baseline", "--no-e2e", "--no-extra-modes")

    full = tmp_path / "full"
    d = _bench("--rows", "1000000", "--steps", "3", "--warmup", "1", "--dump-outputs", str(full), *quiet)
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["dumped_outputs"]["rows"] == 1_000_000 and not d["dumped_outputs"]["sampled"]
    assert sorted(os.listdir(full)) == ["levenshtein.npy", "row_index.npy"]
    got, idx = np.load(full / "levenshtein.npy"), np.load(full / "row_index.npy")
    assert got.dtype == np.float64 and idx.dtype == np.float64 and (idx == np.arange(1_000_000)).all()
    exp = O.batch("levenshtein", *W.host_columns(seed, law, lo, hi, 0, 1_000_000), nthreads=4)
    assert (got.view(np.uint64) == exp.view(np.uint64)).all()

    sample = tmp_path / "sample"
    d = _bench("--rows", "10000000", "--steps", "2", "--warmup", "1", "--dump-outputs", str(sample), *quiet)
    assert d["dumped_outputs"]["sampled"]
    assert sum(os.path.getsize(sample / f) for f in os.listdir(sample)) <= 64_000_000
    got, idx = np.load(sample / "levenshtein.npy"), np.load(sample / "row_index.npy")
    assert got.dtype == np.float64 and len(got) == len(idx) == d["dumped_outputs"]["rows"]
    rows = idx.astype(np.int64)
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < 10_000_000
    import bench
    assert (rows == bench.dump_rows(10_000_000, 1)).all()  # the same seeded rows in every run
    for i in np.linspace(0, len(rows) - 1, 200).astype(np.int64):
        e = O.batch("levenshtein", *W.host_columns(seed, law, lo, hi, int(rows[i]), 1))
        assert got[i].view(np.uint64) == e[0].view(np.uint64), (int(rows[i]), got[i], e[0])


def test_the_metric_is_named_the_same_in_every_run_of_a_frame():
    """`metric` names the measure and the frame only: what varies with a run (step counts, the preheat sized by a timed step) is in its
    own fields, so that runs with different --steps / --warmup are lines of one metric."""
    quiet = ("--rows", "1000000", "--no-cpu-baseline", "--no-e2e", "--no-extra-modes")
    d1 = _bench("--steps", "5", "--warmup", "2", *quiet)
    d2 = _bench("--steps", "9", "--warmup", "0", "--preheat-ms", "80", *quiet)
    assert d1["metric"] == d2["metric"] == "M string-pairs/s, levenshtein, 1 M rows (+ achieved HBM GB/s in roofline)"
    assert (d1["steps"], d1["warmup"], d2["steps"], d2["warmup"]) == (5, 2, 9, 0)
    assert d1["config"]["preheat_ms"] == 40.0 and d2["config"]["preheat_ms"] == 80.0
    assert d1["config"]["preheat_steps"] > 0 and d2["config"]["preheat_steps"] > 0
