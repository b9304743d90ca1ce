#!/usr/bin/env python3
"""Hamming / prefix / postfix / LCSseq distance (strsim_common_distance_device) throughput, device-resident, one JSON line per frame.

Each frame is run through strsim_common_distance_device for the four kinds and, on the same device-resident frame in the same
process right beside them, through strsim_distance_device as "levenshtein" and "indel" (no cutoff anywhere).  Every call is timed
with hipEvents recorded on the context's stream around it, after two warm-up calls (median of 5).  All of these calls wait once for
the stream after their first kernel (include/strsim_amd.h), so their times include that host round trip.

Two conditions are read off frame (a), each with 5 % for noise within one process: hamming, prefix and
postfix take no longer than levenshtein (the same loads, stores and set-up, strictly less work per row), and lcs_seq takes no longer
than indel (the same core).  The line carries them as "ok_vs_levenshtein" / "ok_vs_indel", and the script prints FAIL and exits
non-zero when one does not hold; frame (a)'s line also carries the
fraction of the HBM peak the positional kinds reach, from the bytes the call must move (offsets, strings, output).

Frames: (a) 100 M rows U{1..32} lowercase ASCII (cfg2's generator); (b) 10 M rows Zipf 4..128 bytes (cfg3's law); (c) 1 M rows of
mixed non-ASCII strings of up to 80 bytes; (d) frame (a)'s first column against a literal.  Lines go to stdout and to
profiles/common_bench_lines.jsonl (replaced when every frame is run).

    python bench_support/bench_common.py [frame ...]      (frames: a b c d; default all)
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
OUT = os.path.join(ROOT, "profiles", "common_bench_lines.jsonl")
HBM_PEAK_GBS = 8000.0  # the datasheet figure bench.py's roofline uses
NOISE = 1.05
PARENT = ("levenshtein", "indel")


def host_column(strings):
    o, v = S.pack_strings(strings)
    return (torch.from_numpy(o.view(np.int32)).to(DEV), torch.from_numpy(np.concatenate([v, np.zeros(64, np.uint8)])).to(DEV))


def timed(ctx, what, a, b, n, warmup=2, reps=5):
    stream = torch.cuda.ExternalStream(ctx.stream, device=DEV)
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    ms = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if what in PARENT:
            ctx.distance_device(what, a[0], a[1], b[0], b[1], None, out)
        else:
            ctx.common_distance_device(what, a[0], a[1], b[0], b[1], None, out)
        e1.record(stream)
        ctx.synchronize()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), int(ctx.last_wave_rows) if what not in PARENT else None


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


def moved_bytes(a, b, n):
    """what a distance call must read and write: both offset columns, the bytes of the strings, one uint32 a row"""
    total = 4 * n
    for off, _ in (a, b):
        total += 4 * off.numel() + ((int(off[-1].item()) - int(off[0].item())) & 0xFFFFFFFF)  # (u32 bits in an i32 tensor)
    return total


def main():
    frames = sys.argv[1:] or ["a", "b", "c", "d"]
    lines = []
    with S.Context(0) as ctx:
        for f in frames:
            desc, a, b, n = frame(f)
            line = {"bench": "common", "frame": f, "desc": desc, "rows": n, "device": torch.cuda.get_device_name(0)}
            ms = {}
            for what in PARENT + S.COMMON_KINDS:
                ms[what], wave_rows = timed(ctx, what, a, b, n)
                line[what + "_ms"] = round(ms[what], 4)
                line[what + "_mpairs_s"] = round(n / ms[what] / 1e3, 1)
                if wave_rows is not None:
                    line[what + "_wave_rows"] = wave_rows
            for kind in ("hamming", "prefix", "postfix"):
                line[kind + "_over_levenshtein_time"] = round(ms[kind] / ms["levenshtein"], 3)
            line["lcs_seq_over_indel_time"] = round(ms["lcs_seq"] / ms["indel"], 3)
            if f == "a":
                line["ok_vs_levenshtein"] = all(ms[k] <= NOISE * ms["levenshtein"] for k in ("hamming", "prefix", "postfix"))
                line["ok_vs_indel"] = ms["lcs_seq"] <= NOISE * ms["indel"]
                gb = moved_bytes(a, b, n) / 1e9
                line["moved_gb"] = round(gb, 3)
                for kind in ("hamming", "prefix", "postfix"):
                    line[kind + "_hbm_frac"] = round(gb / (ms[kind] / 1e3) / HBM_PEAK_GBS, 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del a, b
            torch.cuda.empty_cache()
    if sorted(frames) == ["a", "b", "c", "d"]:
        with open(OUT, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")
    failed = [c for ln in lines for c in ("ok_vs_levenshtein", "ok_vs_indel") if ln.get(c) is False]
    for c in failed:
        print("FAIL: condition %s of frame (a) does not hold" % c, flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
