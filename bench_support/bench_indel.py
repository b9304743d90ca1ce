#!/usr/bin/env python3
"""Indel (LCS) similarity (measure 8) throughput, device-resident, one JSON line per frame.

Each frame is run through strsim_pairs_device as "indel" and, on the same device-resident frame in the same process, as "osa" and as
"levenshtein".  Every call is timed with hipEvents recorded on the context's stream around it (median of the timed repetitions).  An
Indel call, like an OSA call, waits once for the stream after its first kernel (include/strsim_amd.h), so its time includes that
host round trip.  The comparison that matters is indel against osa within one run: the OSA kernels are the ones this measure's
tiers were derived from.

Frames: (a) 100 M rows U{1..32} lowercase ASCII (cfg2's generator); (b) 10 M rows Zipf 4..128 bytes (cfg3's law); (c) 1 M rows of
mixed non-ASCII strings of up to 80 bytes; (d) frame (a)'s first column against a literal.  Lines go to stdout and to
profiles/indel_bench_lines.jsonl (replaced when every frame is run).

    python bench_support/bench_indel.py [frame ...]      (frames: a b c d; default all)
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
OUT = os.path.join(ROOT, "profiles", "indel_bench_lines.jsonl")


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
            reps = 10 if n >= 10_000_000 else 20
            res = {}
            for m in ("levenshtein", "osa", "indel"):
                ms, wave_rows = timed(ctx, m, a, b, n, 3, reps)
                res[m] = (ms, wave_rows)
            line = {"bench": "indel", "frame": f, "desc": desc, "rows": n,
                    "indel_ms": round(res["indel"][0], 4), "indel_mpairs_s": round(n / res["indel"][0] / 1e3, 1),
                    "indel_wave_rows": int(res["indel"][1]),
                    "osa_ms": round(res["osa"][0], 4), "osa_mpairs_s": round(n / res["osa"][0] / 1e3, 1),
                    "osa_wave_rows": int(res["osa"][1]),
                    "lev_ms": round(res["levenshtein"][0], 4), "lev_mpairs_s": round(n / res["levenshtein"][0] / 1e3, 1),
                    "indel_over_osa_time": round(res["indel"][0] / res["osa"][0], 3),
                    "indel_over_lev_rate": round(res["levenshtein"][0] / res["indel"][0], 3), "device": torch.cuda.get_device_name(0)}
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
