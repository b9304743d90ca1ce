#!/usr/bin/env python3
"""q-gram similarity (strsim_qgram_device) throughput, device-resident, one JSON line per frame.

Each frame is run through strsim_qgram_device as sorensen_dice at q = 2 (the figure with a condition), at q = 3 and in set mode, and,
on the same device-resident frame in the same process, through strsim_pairs_device as "indel".  Every call is timed with hipEvents
recorded on the context's stream around it (median of 10 timed repetitions behind 3 warm-ups).  A q-gram call, like an Indel call,
waits once for the stream after its first kernel (include/strsim_amd.h), so its time includes that host round trip.  The comparison
that matters is qgram_sorensen_dice(q = 2) against indel within one run, on frame (a): both kernels load per-lane windows, build seven
planes and run a wave to its longest text, and Indel's kernels are not touched by this measure.

Frames: (a) 100 M rows U{1..32} lowercase ASCII (cfg2's generator); (b) 10 M rows Zipf 4..128 bytes (cfg3's law); (c) 1 M rows of
mixed non-ASCII strings of up to 80 bytes; (d) frame (a)'s first column against a literal.  Lines go to stdout and to
profiles/qgram_bench_lines.jsonl (replaced when every frame is run).

    python bench_support/bench_qgram.py [frame ...]      (frames: a b c d; default all)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gen
import strsim_amd as S
from bench_support import workload as W

DEV = torch.device("cuda", 0)
OUT = os.path.join(ROOT, "profiles", "qgram_bench_lines.jsonl")
WARMUP, REPS = 3, 10


def host_column(strings):
    o, v = S.pack_strings(strings)
    return (torch.from_numpy(o.view(np.int32)).to(DEV), torch.from_numpy(np.concatenate([v, np.zeros(64, np.uint8)])).to(DEV))


def timed(ctx, call, n):
    """call(out) enqueues on the context's stream -> (median ms, last_wave_rows)."""
    stream = torch.cuda.ExternalStream(ctx.stream, device=DEV)
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    ms = []
    for r in range(WARMUP + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call(out)
        e1.record(stream)
        ctx.synchronize()
        e1.synchronize()
        if r >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), ctx.last_wave_rows


def frame(name):
    if name in ("a", "d"):
        _, _, law, lo, hi, seed = W.CONFIGS["cfg2"]
        oa, va, ob, vb, _, _ = W.device_columns(seed, law, lo, hi, 0, 100_000_000, DEV)
        if name == "a":
            return "100M U{1..32} ASCII (cfg2)", (oa, va), (ob, vb), 100_000_000
        lit = host_column(["jonathan"])
        return "100M U{1..32} ASCII x literal 'jonathan'", (oa, va), lit, 100_000_000
    if name == "b":
        _, _, law, lo, hi, seed = W.CONFIGS["cfg3"]
        oa, va, ob, vb, _, _ = W.device_columns(seed, law, lo, hi, 0, 10_000_000, DEV)
        return "10M Zipf 4..128 bytes (cfg3 law)", (oa, va), (ob, vb), 10_000_000
    A, B = gen.pairs(31, 1_000_000, gen.MIXED, 0, 80, max_bytes=80)
    return "1M mixed non-ASCII <= 80 bytes", host_column(A), host_column(B), 1_000_000


def main():
    frames = sys.argv[1:] or ["a", "b", "c", "d"]
    lines = []
    with S.Context(0) as ctx:
        for f in frames:
            desc, a, b, n = frame(f)
            runs = {
                "indel": lambda out: ctx.pairs_device("indel", a[0], a[1], b[0], b[1], out),
                "dice_q2": lambda out: ctx.qgram_device("sorensen_dice", a[0], a[1], b[0], b[1], 2, True, out),
                "dice_q3": lambda out: ctx.qgram_device("sorensen_dice", a[0], a[1], b[0], b[1], 3, True, out),
                "dice_q2_set": lambda out: ctx.qgram_device("sorensen_dice", a[0], a[1], b[0], b[1], 2, False, out),
            }
            res = {k: timed(ctx, call, n) for k, call in runs.items()}
            line = {"bench": "qgram", "frame": f, "desc": desc, "rows": n}
            for k, (ms, wave_rows) in res.items():
                line[k + "_ms"] = round(ms, 4)
                line[k + "_mpairs_s"] = round(n / ms / 1e3, 1)
                line[k + "_wave_rows"] = int(wave_rows)
            line["dice_q2_over_indel_time"] = round(res["dice_q2"][0] / res["indel"][0], 3)
            line["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del a, b, runs
            torch.cuda.empty_cache()
    if sorted(frames) == ["a", "b", "c", "d"]:
        with open(OUT, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
