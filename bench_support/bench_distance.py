#!/usr/bin/env python3
"""Bounded edit distance throughput (strsim_distance_device), device-resident, one JSON line per frame, measure and cutoff.

Each frame is run through strsim_distance_device and, on the same device-resident frame right beside it, through the matching
similarity (strsim_pairs_device, same measure).  Every call is timed with hipEvents recorded on the context's stream around it (median
of the timed repetitions).  A distance call waits once for the stream after its first kernel (include/strsim_amd.h), so its time
includes that host round trip.

Frames: (a) 100 M rows U{1..32} lowercase ASCII (cfg2's generator); (b) 10 M rows Zipf 4..128 bytes (cfg3's law); (c) 1 M rows of
mixed non-ASCII strings of up to 80 bytes; (d) 1 M pairs of 400..1000 ASCII bytes, half near duplicates (about 1 % random edits),
half unrelated, with max_distance unbounded, 16 and 4.  Lines go to stdout and to profiles/distance_bench_lines.jsonl (replaced
when every frame is run).

    python bench_support/bench_distance.py [frame ...] [--cutoffs K,K,...]      (frames: a b c d; default all)

--cutoffs replaces frame (d)'s cutoffs (`unbounded` or an integer); the lines then go to stdout only.
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
OUT = os.path.join(ROOT, "profiles", "distance_bench_lines.jsonl")


def host_column(strings):
    o, v = S.pack_strings(strings)
    return (torch.from_numpy(o.view(np.int32)).to(DEV), torch.from_numpy(np.concatenate([v, np.zeros(64, np.uint8)])).to(DEV))


def timed(ctx, call, warmup, reps):
    stream = torch.cuda.ExternalStream(ctx.stream, device=DEV)
    ms = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        ctx.synchronize()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def long_pairs(n, seed=41):
    """n pairs of 400..1000 ASCII bytes: even rows near duplicates (about 1 % random edits), odd rows unrelated."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(400, 1001, n)
    letters = np.frombuffer(gen.ASCII_LOWER.encode(), dtype=np.uint8)
    A, B = [], []
    for i in range(n):
        a = letters[rng.integers(0, 26, lens[i])]
        if i % 2 == 0:
            b = a.copy()
            e = max(1, lens[i] // 100)
            pos = rng.integers(0, lens[i], e)
            b[pos] = letters[rng.integers(0, 26, e)]
            b = b.tobytes()
            for _ in range(int(rng.integers(0, 3))):  # a few indels besides the substitutions
                p = int(rng.integers(0, len(b)))
                b = b[:p] + b[p + 1:] if rng.random() < 0.5 else b[:p] + b"q" + b[p:]
        else:
            b = letters[rng.integers(0, 26, rng.integers(400, 1001))].tobytes()
        A.append(a.tobytes())
        B.append(b)
    return A, B


def frame(name, d_cutoffs=(None, 16, 4)):
    if name == "a":
        _, _, law, lo, hi, seed = W.CONFIGS["cfg2"]
        oa, va, ob, vb, _, _ = W.device_columns(seed, law, lo, hi, 0, 100_000_000, DEV)
        return "100M U{1..32} ASCII (cfg2)", (oa, va), (ob, vb), 100_000_000, (None,)
    if name == "b":
        _, _, law, lo, hi, seed = W.CONFIGS["cfg3"]
        oa, va, ob, vb, _, _ = W.device_columns(seed, law, lo, hi, 0, 10_000_000, DEV)
        return "10M Zipf 4..128 bytes (cfg3 law)", (oa, va), (ob, vb), 10_000_000, (None,)
    if name == "c":
        A, B = gen.pairs(31, 1_000_000, gen.MIXED, 0, 80, max_bytes=80)
        return "1M mixed non-ASCII <= 80 bytes", host_column(A), host_column(B), 1_000_000, (None,)
    A, B = long_pairs(1_000_000)
    return "1M pairs 400..1000 ASCII bytes, half ~1% edits, half unrelated", host_column(A), host_column(B), 1_000_000, d_cutoffs


def main():
    args = sys.argv[1:]
    d_cutoffs = None
    if "--cutoffs" in args:
        i = args.index("--cutoffs")
        d_cutoffs = tuple(None if c == "unbounded" else int(c) for c in args[i + 1].split(","))
        del args[i:i + 2]
    frames = args or ["a", "b", "c", "d"]
    lines = []
    with S.Context(0) as ctx:
        for f in frames:
            desc, a, b, n, cutoffs = frame(f, d_cutoffs) if d_cutoffs else frame(f)
            torch.cuda.synchronize()  # (uploads ran on torch's stream; the calls run on the context's)
            reps = 10 if n >= 10_000_000 else 5
            sim = torch.empty(n, dtype=torch.float64, device=DEV)
            dist = torch.empty(n, dtype=torch.int32, device=DEV)
            for m in ("levenshtein", "osa"):
                sim_ms = timed(ctx, lambda: ctx.pairs_device(m, a[0], a[1], b[0], b[1], sim), 2, reps)
                for k in cutoffs:
                    ms = timed(ctx, lambda: ctx.distance_device(m, a[0], a[1], b[0], b[1], k, dist), 2, reps)
                    line = {"bench": "distance", "frame": f, "desc": desc, "rows": n, "measure": m,
                            "max_distance": "unbounded" if k is None else k,
                            "dist_ms": round(ms, 4), "dist_mpairs_s": round(n / ms / 1e3, 1),
                            "sim_ms": round(sim_ms, 4), "sim_mpairs_s": round(n / sim_ms / 1e3, 1),
                            "dist_over_sim_rate": round(sim_ms / ms, 3), "device": torch.cuda.get_device_name(0)}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
            del a, b, sim, dist
            torch.cuda.empty_cache()
    if sorted(frames) == ["a", "b", "c", "d"] and d_cutoffs is None:
        with open(OUT, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
