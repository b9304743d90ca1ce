#!/usr/bin/env python3
"""Unrestricted Damerau-Levenshtein (strsim_damerau_device) throughput, device-resident, one JSON line per frame.

Each frame is run through strsim_damerau_device and, on the same device-resident frame in the same process right beside it,
through strsim_pairs_device as "osa".  Every call is timed with hipEvents recorded on the context's stream around it, after a
warm-up (median of the timed repetitions).  Both calls wait once for the stream after their first kernel (include/strsim_amd.h), so
their times include that host round trip.  The comparison is a cell DP against a bit-parallel column step: DESIGN.md section 26.

Frames: (a) 100 M rows U{1..32} lowercase ASCII (cfg2's generator); (b) 10 M rows Zipf 4..128 bytes (cfg3's law); (c) 1 M rows of
mixed non-ASCII strings of up to 80 bytes; (d) frame (a)'s first column against a literal.  Lines go to stdout and to
profiles/damerau_bench_lines.jsonl (replaced when every frame is run).

    python bench_support/bench_damerau.py [frame ...]      (frames: a b c d; default all)
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
OUT = os.path.join(ROOT, "profiles", "damerau_bench_lines.jsonl")


def host_column(strings):
    o, v = S.pack_strings(strings)
    return (torch.from_numpy(o.view(np.int32)).to(DEV), torch.from_numpy(np.concatenate([v, np.zeros(64, np.uint8)])).to(DEV))


def timed(ctx, measure, a, b, n, warmup, reps):
    stream = torch.cuda.ExternalStream(ctx.stream, device=DEV)
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    ms = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if measure == "damerau_levenshtein":
            ctx.damerau_device(a[0], a[1], b[0], b[1], out)
        else:
            ctx.pairs_device(measure, a[0], a[1], b[0], b[1], out)
        e1.record(stream)
        ctx.synchronize()
        e1.synchronize()
        if r >= warmup:
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
            reps = 5 if n >= 10_000_000 else 10
            res = {}
            for m in ("osa", "damerau_levenshtein"):
                ms, wave_rows = timed(ctx, m, a, b, n, 2, reps)
                res[m] = (ms, wave_rows)
            dl, osa = res["damerau_levenshtein"], res["osa"]
            line = {"bench": "damerau", "frame": f, "desc": desc, "rows": n,
                    "dl_ms": round(dl[0], 4), "dl_mpairs_s": round(n / dl[0] / 1e3, 1), "dl_wave_rows": int(dl[1]),
                    "osa_ms": round(osa[0], 4), "osa_mpairs_s": round(n / osa[0] / 1e3, 1), "osa_wave_rows": int(osa[1]),
                    "dl_over_osa_time": round(dl[0] / osa[0], 2), "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del a, b
            torch.cuda.empty_cache()
    if sorted(frames) == ["a", "b", "c", "d"]:
        with open(OUT, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
