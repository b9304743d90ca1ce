#!/usr/bin/env python3
"""Best match (strsim_best_match_device) throughput, one JSON line per run, device-resident.

Frames: (a) 100 k queries x 10 k candidates of cfg2's generator (U{1..32} ASCII), every measure, k = 1 and 16; (b) 1 M x 1 k;
(c) 10 k x 100 k; (d) a Cyrillic / long-ASCII mix (the fallback).  Each line: N*M / time of the call (hipEvents around it on the
context's stream), and beside it, in the same process, what a user has today on the GPU: the cross product materialised on the
device and run through strsim_pairs_device.  That baseline is timed on a slice of the cross product (`xp_pairs_timed` pairs:
whole query rows x all candidates) and reported as pairs/s and as the time it would take for N*M pairs; materialising the
product and the arg-max afterwards are not counted, which flatters it.

    python bench_support/bench_best_match.py [frame ...]      (frames: a b c d; default all)
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import strsim_amd as S
from strsim_amd._lib import check, lib
from bench_support import workload as W

DEV = torch.device("cuda", 0)
XP_PAIRS = 20_000_000


def cfg2_column(n, seed_row0):
    _, _, law, lo, hi, seed = W.CONFIGS["cfg2"]
    off, val, _, _, _, _ = W.device_columns(seed, law, lo, hi, seed_row0, n, DEV)
    return off, val


def host_column(strings):
    o, v = S.pack_strings(strings)
    return (torch.from_numpy(o.view(np.int32)).to(DEV), torch.from_numpy(np.concatenate([v, np.zeros(64, np.uint8)])).to(DEV))


def lengths(off):
    return (off[1:].to(torch.int64) & 0xFFFFFFFF) - (off[:-1].to(torch.int64) & 0xFFFFFFFF)


def cross_slice(qoff, qval, coff, cval, nq):
    """rows 0 .. nq-1 of the queries x every candidate, as two materialised pair columns"""
    m = coff.numel() - 1
    lq, lc = lengths(qoff[: nq + 1]), lengths(coff)
    sq, sc = qoff[:nq].to(torch.int64) & 0xFFFFFFFF, coff[:-1].to(torch.int64) & 0xFFFFFFFF
    cols = []
    for starts, lens in ((sq.repeat_interleave(m), lq.repeat_interleave(m)), (sc.repeat(nq), lc.repeat(nq))):
        o = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=DEV)
        torch.cumsum(lens, 0, out=o[1:])
        tot = int(o[-1].item())
        src = torch.repeat_interleave(starts - o[:-1], lens) + torch.arange(tot, device=DEV)
        vals = (qval if len(cols) == 0 else cval)[src]
        cols.append((o.to(torch.int32), torch.cat([vals, torch.zeros(64, dtype=torch.uint8, device=DEV)])))
        del src
    return cols


def timed(ctx, fn, reps):
    st = torch.cuda.current_stream()
    fn()
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    ctx.synchronize()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps / 1e3


def run_frame(ctx, frame, measure, k, q, c, reps=3):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    idx = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    sc = torch.empty((nq, k), dtype=torch.float64, device=DEV)
    mid = S.MEASURE_ID[measure]

    def bm():
        check(lib().strsim_best_match_device(ctx._h, mid, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc,
                                             k, float("-inf"), idx.data_ptr(), sc.data_ptr()))
    t = timed(ctx, bm, reps)
    xq = max(1, min(nq, XP_PAIRS // nc))
    (ao, av), (bo, bv) = cross_slice(qoff, qval, coff, cval, xq)
    out = torch.empty(xq * nc, dtype=torch.float64, device=DEV)
    tx = timed(ctx, lambda: ctx.pairs_device(measure, ao, av, bo, bv, out=out), reps)
    del ao, av, bo, bv
    # the slice's arg-max agrees with the best match of those rows (k = 1: first index of the maximum)
    agree = None
    if k == 1:
        best = out.view(xq, nc).argmax(dim=1)
        agree = bool(torch.equal(best.to(torch.int32), idx[:xq, 0]))
    pairs = nq * nc
    xp_rate = xq * nc / tx
    line = {"bench": "best_match", "frame": frame, "measure": measure, "k": k, "queries": nq, "candidates": nc,
            "kernel_ms": round(t * 1e3, 4), "pairs_per_s": round(pairs / t, 1), "xp_pairs_timed": xq * nc,
            "xp_pairs_per_s": round(xp_rate, 1), "xp_ms_for_frame": round(pairs / xp_rate * 1e3, 4),
            "speedup_vs_xp": round((pairs / xp_rate) / t, 3), "xp_argmax_agrees": agree}
    print(json.dumps(line), flush=True)


def mixed_strings(seed, n):
    rng = random.Random(seed)
    cyr = "абвгдеёжзийклмнопрстуфхцчшщыэюя"
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.4:
            out.append("".join(rng.choice(cyr) for _ in range(rng.randint(1, 24))))
        elif r < 0.7:
            out.append("".join(rng.choice("abcdefghij") for _ in range(rng.randint(33, 200))))
        else:
            out.append("".join(rng.choice("abcdefghij") for _ in range(rng.randint(0, 32))))
    return out


def main():
    frames = sys.argv[1:] or ["a", "b", "c", "d"]
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = S.Context(0, stream=st.cuda_stream)
    for f in frames:
        if f == "a":
            q, c = cfg2_column(100_000, 0), cfg2_column(10_000, 200_000)
            for m in S.MEASURES:
                for k in (1, 16):
                    run_frame(ctx, "a", m, k, q, c)
        elif f == "b":
            q, c = cfg2_column(1_000_000, 0), cfg2_column(1_000, 2_000_000)
            for m in ("levenshtein", "jaro_winkler"):
                run_frame(ctx, "b", m, 1, q, c)
        elif f == "c":
            q, c = cfg2_column(10_000, 0), cfg2_column(100_000, 200_000)
            for m in ("levenshtein", "jaro_winkler"):
                for k in (1, 16):
                    run_frame(ctx, "c", m, k, q, c)
        elif f == "d":
            q, c = host_column(mixed_strings(1, 2_000)), host_column(mixed_strings(2, 1_000))
            for m in ("levenshtein", "jaro_winkler"):
                run_frame(ctx, "d", m, 1, q, c, reps=1)
    ctx.close()


if __name__ == "__main__":
    main()
