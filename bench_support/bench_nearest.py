#!/usr/bin/env python3
"""Nearest match (strsim_nearest_device) throughput, one JSON line per run, device-resident.

Frames: (a) 100 k queries x 10 k candidates of cfg2's generator (U{1..32} ASCII; best match's frame (a)), both measures, k = 1 and
16, max_distance unbounded, 4, 2, 1; (b) near duplicates: 10 k cfg2 candidates, 100 k queries that are a random candidate with 0..3
random edits (insert, delete, substitute, adjacent swap), k = 1, unbounded and 2; (c) a Cyrillic / long-ASCII mix, 2 k x 1 k (the
fallback path).  Each line: N*M / time of the call (hipEvents around it on the context's stream) and, as the baseline in the same
process on the same device-resident frame, strsim_best_match_device(levenshtein, k = 1).  `window_pairs` is the number of pairs
the static window admits (each wave of 64 length-ordered queries against the candidate lengths within max_distance of its own),
counted on the CPU from the two length histograms.

    python bench_support/bench_nearest.py [--out FILE] [frame ...]      (frames: a b c; default all; lines are appended to FILE,
                                                                           default profiles/nearest_bench_lines.jsonl)
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
from strsim_amd._lib import DISTANCE_UNBOUNDED as U, check, lib
from bench_support import workload as W

DEV = torch.device("cuda", 0)


def cfg2_column(n, seed_row0):
    _, _, law, lo, hi, seed = W.CONFIGS["cfg2"]
    off, val, _, _, _, _ = W.device_columns(seed, law, lo, hi, seed_row0, n, DEV)
    return off, val


def host_column(strings):
    o, v = S.pack_strings(strings)
    return (torch.from_numpy(o.view(np.int32)).to(DEV), torch.from_numpy(np.concatenate([v, np.zeros(64, np.uint8)])).to(DEV))


def to_strings(col):
    off, val = col
    o = off.cpu().numpy().view(np.uint32).astype(np.int64)
    v = val.cpu().numpy().tobytes()
    return [v[o[i]:o[i + 1]].decode() for i in range(o.size - 1)]


def near_duplicates(seed, cands, n, alphabet="abcdefghijklmnopqrstuvwxyz"):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = list(rng.choice(cands))
        for _ in range(rng.randint(0, 3)):
            op = rng.randrange(4)
            p = rng.randrange(len(s) + 1)
            if op == 0:
                s.insert(p, rng.choice(alphabet))
            elif op == 1 and s:
                del s[min(p, len(s) - 1)]
            elif op == 2 and s:
                s[min(p, len(s) - 1)] = rng.choice(alphabet)
            elif op == 3 and len(s) >= 2:
                p = min(p, len(s) - 2)
                s[p], s[p + 1] = s[p + 1], s[p]
        out.append("".join(s))
    return out


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


def byte_lengths(col):
    o = col[0].cpu().numpy().view(np.uint32).astype(np.int64)
    return np.diff(o)


def window_pairs(q, c, md):
    """pairs the static window admits: the lane class (<= 32 bytes; these frames' fast strings are ASCII) in waves of 64"""
    lq, lc = np.sort(byte_lengths(q)), byte_lengths(c)
    lq = lq[lq <= 32]
    hist = np.bincount(lc[lc <= 32], minlength=33)
    cum = np.concatenate([[0], np.cumsum(hist)])
    k = 10 ** 9 if md == U else md
    total = 0
    for w0 in range(0, lq.size, 64):
        lmin, lmax = int(lq[w0]), int(lq[min(w0 + 64, lq.size) - 1])
        lo, hi = max(0, lmin - k), min(32, lmax + k)
        total += (min(w0 + 64, lq.size) - w0) * int(cum[hi + 1] - cum[lo])
    return total


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


def best_match_ms(ctx, q, c, reps):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    idx = torch.empty((nq, 1), dtype=torch.int32, device=DEV)
    sc = torch.empty((nq, 1), dtype=torch.float64, device=DEV)

    def bm():
        check(lib().strsim_best_match_device(ctx._h, 0, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc,
                                             1, float("-inf"), idx.data_ptr(), sc.data_ptr()))
    return timed(ctx, bm, reps) * 1e3


def run(ctx, out, frame, measure, k, md, q, c, bm_ms, reps=3):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    idx = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    dist = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    mid = S.MEASURE_ID[measure]

    def nm():
        check(lib().strsim_nearest_device(ctx._h, mid, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc,
                                          k, md, idx.data_ptr(), dist.data_ptr()))
    t = timed(ctx, nm, reps)
    pairs = nq * nc
    wp = window_pairs(q, c, md)
    line = {"bench": "nearest", "frame": frame, "measure": measure, "k": k, "max_distance": None if md == U else md,
            "queries": nq, "candidates": nc, "kernel_ms": round(t * 1e3, 4), "pairs_per_s": round(pairs / t, 1),
            "window_pairs": wp, "window_fraction": round(wp / pairs, 4), "best_match_lev_k1_ms": round(bm_ms, 4),
            "vs_best_match": round(t * 1e3 / bm_ms, 3)}
    print(json.dumps(line), flush=True)
    out.write(json.dumps(line) + "\n")
    out.flush()


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "nearest_bench_lines.jsonl")
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    frames = args or ["a", "b", "c"]
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = S.Context(0, stream=st.cuda_stream)
    with open(path, "a") as out:
        for f in frames:
            if f == "a":
                q, c = cfg2_column(100_000, 0), cfg2_column(10_000, 200_000)
                bm = best_match_ms(ctx, q, c, 3)
                for m in S.DISTANCE_MEASURES:
                    for k in (1, 16):
                        for md in (U, 4, 2, 1):
                            run(ctx, out, "a", m, k, md, q, c, bm)
            elif f == "b":
                c = cfg2_column(10_000, 200_000)
                q = host_column(near_duplicates(7, to_strings(c), 100_000))
                bm = best_match_ms(ctx, q, c, 3)
                for m in S.DISTANCE_MEASURES:
                    for md in (U, 2):
                        run(ctx, out, "b", m, 1, md, q, c, bm)
            elif f == "c":
                q, c = host_column(mixed_strings(1, 2_000)), host_column(mixed_strings(2, 1_000))
                bm = best_match_ms(ctx, q, c, 1)
                for m in S.DISTANCE_MEASURES:
                    run(ctx, out, "c", m, 1, U, q, c, bm, reps=1)
    ctx.close()


if __name__ == "__main__":
    main()
