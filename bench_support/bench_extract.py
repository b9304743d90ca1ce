#!/usr/bin/env python3
"""Extract (strsim_extract_device) throughput, one JSON line per run, device-resident.

Every call is timed with hipEvents recorded on the context's stream around it (median of 10 timed repetitions behind 3 warm-ups).
The baseline is always code that extract does not touch, timed in the same process on the same device-resident frame.

Frames: (a) 100 k queries x 10 k candidates of cfg2's generator (U{1..32} ASCII; best match's and nearest's frame (a)), scorer
ratio, k = 1 and 16, score_cutoff none, 0.5, 0.8, 0.9; baseline strsim_best_match_device(levenshtein, k = 1).  `window_pairs` is
the number of pairs the static window admits (each wave of 64 length-ordered queries against the candidate lengths whose best
possible score reaches the cutoff), counted on the CPU from the two length histograms.  (b) near duplicates: 10 k cfg2 candidates,
100 k queries that are a random candidate with 0..3 random edits, k = 1, cutoff none and 0.8; the same baseline.  (c) 100 k x 10 k
of the token frame (tests/token_ref.py's generator, 1-4 tokens), scorer token_sort_ratio; baseline: scorer ratio over the columns
normalised beforehand by strsim_token_sort_device.  (slice) 2 000 queries of frame (a) against its 10 k candidates (2 * 10^7 pairs)
through extract(ratio, k = 1); baseline: the slice's cross product materialised and scored by strsim_pairs_device(STRSIM_INDEL),
which is what a caller without extract does (the gather that builds the cross product is not timed).

    python bench_support/bench_extract.py [--out FILE] [frame ...]      (frames: a b c slice; default all; lines are appended to
                                                                           FILE, default profiles/extract_bench_lines.jsonl)
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

import strsim_amd as S
import token_ref
from strsim_amd._lib import check, lib
from bench_support.bench_nearest import DEV, byte_lengths, cfg2_column, host_column, near_duplicates, to_strings

INDEL, TOKEN_SORT = S.MEASURE_ID["indel"], S.MEASURE_ID["token_sort_ratio"]


def timed(ctx, call, warmup=3, reps=10):
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


def ub(lq, lc):
    """the best score a candidate of lc bytes can reach against a query of lq bytes: the library's two f64 operations"""
    return 1.0 if lq + lc == 0 else 1.0 - (float(abs(lq - lc)) / float(lq + lc))


def window_pairs(q, c, cutoff):
    """pairs the static window admits: the lane class (<= 32 bytes; these frames' fast strings are ASCII) in waves of 64"""
    lq, lc = np.sort(byte_lengths(q)), byte_lengths(c)
    lq = lq[lq <= 32]
    hist = np.bincount(lc[lc <= 32], minlength=33)
    cum = np.concatenate([[0], np.cumsum(hist)])
    if cutoff is not None and cutoff > 1.0:
        return 0
    total = 0
    for w0 in range(0, lq.size, 64):
        lmin, lmax = int(lq[w0]), int(lq[min(w0 + 64, lq.size) - 1])
        lo, hi = lmin, lmax
        while lo > 0 and (cutoff is None or ub(lmin, lo - 1) >= cutoff):
            lo -= 1
        while hi < 32 and (cutoff is None or ub(lmax, hi + 1) >= cutoff):
            hi += 1
        total += (min(w0 + 64, lq.size) - w0) * int(cum[hi + 1] - cum[lo])
    return total


def best_match_ms(ctx, q, c):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    idx = torch.empty((nq, 1), dtype=torch.int32, device=DEV)
    sc = torch.empty((nq, 1), dtype=torch.float64, device=DEV)

    def bm():
        check(lib().strsim_best_match_device(ctx._h, 0, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc,
                                             1, float("-inf"), idx.data_ptr(), sc.data_ptr()))
    return timed(ctx, bm)


def extract_ms(ctx, scorer, q, c, k, cutoff):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    idx = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    sc = torch.empty((nq, k), dtype=torch.float64, device=DEV)
    cut = float("-inf") if cutoff is None else float(cutoff)

    def ex():
        check(lib().strsim_extract_device(ctx._h, scorer, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc,
                                          k, cut, idx.data_ptr(), sc.data_ptr()))
    return timed(ctx, ex)


def token_sorted(ctx, col):
    """the column normalised by strsim_token_sort_device (outside every timed region)"""
    off, val = col
    rows = off.numel() - 1
    cap = val.numel()
    out_off = torch.empty(rows + 1, dtype=torch.int32, device=DEV)
    out_val = torch.zeros(cap + 64, dtype=torch.uint8, device=DEV)
    check(lib().strsim_token_sort_device(ctx._h, off.data_ptr(), val.data_ptr(), rows, out_off.data_ptr(), out_val.data_ptr(), cap))
    ctx.synchronize()
    return out_off, out_val


def cross_product(q, c):
    """the explicit pair columns of every (query, candidate): what strsim_pairs_device needs without a search entry point"""
    def lengths(col):
        o = col[0].to(torch.int64) & 0xFFFFFFFF
        return o[:-1], o[1:] - o[:-1]

    def gather(col, rows):
        start, ln = lengths(col)
        s, l = start[rows], ln[rows]
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(l, 0)])
        pos = torch.arange(int(off[-1]), device=DEV) - torch.repeat_interleave(off[:-1], l) + torch.repeat_interleave(s, l)
        val = torch.cat([col[1][pos], torch.zeros(64, dtype=torch.uint8, device=DEV)])
        return off.to(torch.int32).contiguous(), val.contiguous()
    nq, nc = q[0].numel() - 1, c[0].numel() - 1
    qi = torch.arange(nq, device=DEV).repeat_interleave(nc)
    ci = torch.arange(nc, device=DEV).repeat(nq)
    return gather(q, qi), gather(c, ci)


def emit(out, line):
    print(json.dumps(line), flush=True)
    out.write(json.dumps(line) + "\n")
    out.flush()


def run(ctx, out, frame, scorer, k, cutoff, q, c, base_ms, base_name, with_window=False):
    t = extract_ms(ctx, scorer, q, c, k, cutoff)
    nq, nc = q[0].numel() - 1, c[0].numel() - 1
    pairs = nq * nc
    line = {"bench": "extract", "frame": frame, "scorer": "ratio" if scorer == INDEL else "token_sort_ratio", "k": k,
            "score_cutoff": cutoff, "queries": nq, "candidates": nc, "call_ms": round(t, 4), "pairs_per_s": round(pairs / (t / 1e3), 1),
            "baseline": base_name, "baseline_ms": round(base_ms, 4), "vs_baseline": round(t / base_ms, 3)}
    if with_window:
        wp = window_pairs(q, c, cutoff)
        line["window_pairs"] = wp
        line["window_fraction"] = round(wp / pairs, 4)
    emit(out, line)
    return t


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "extract_bench_lines.jsonl")
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    frames = args or ["a", "b", "c", "slice"]
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = S.Context(0, stream=st.cuda_stream)
    with open(path, "a") as out:
        for f in frames:
            if f == "a":
                q, c = cfg2_column(100_000, 0), cfg2_column(10_000, 200_000)
                bm = best_match_ms(ctx, q, c)
                for k in (1, 16):
                    for cut in (None, 0.5, 0.8, 0.9):
                        run(ctx, out, "a", INDEL, k, cut, q, c, bm, "best_match_lev_k1", True)
            elif f == "b":
                c = cfg2_column(10_000, 200_000)
                q = host_column(near_duplicates(7, to_strings(c), 100_000))
                bm = best_match_ms(ctx, q, c)
                for cut in (None, 0.8):
                    run(ctx, out, "b", INDEL, 1, cut, q, c, bm, "best_match_lev_k1", True)
            elif f == "c":
                A, B = token_ref.gen_frame(2024, 100_000)
                q, c = host_column(A), host_column(B[:10_000])
                qs, cs = token_sorted(ctx, q), token_sorted(ctx, c)
                for k, cut in ((1, None), (1, 0.8), (16, None)):
                    base = extract_ms(ctx, INDEL, qs, cs, k, cut)
                    run(ctx, out, "c", TOKEN_SORT, k, cut, q, c, base, "extract_ratio_prenormalised")
            elif f == "slice":
                qa, c = cfg2_column(100_000, 0), cfg2_column(10_000, 200_000)
                q = host_column(to_strings(qa)[:2_000])
                (ao, av), (bo, bv) = cross_product(q, c)
                n = ao.numel() - 1
                res = torch.empty(n, dtype=torch.float64, device=DEV)
                torch.cuda.synchronize()

                def pairs():
                    check(lib().strsim_pairs_device(ctx._h, INDEL, ao.data_ptr(), av.data_ptr(), n, bo.data_ptr(), bv.data_ptr(), n,
                                                    res.data_ptr(), n))
                base = timed(ctx, pairs)
                run(ctx, out, "slice", INDEL, 1, None, q, c, base, "pairs_device_indel_cross_product")
                run(ctx, out, "slice", INDEL, 16, None, q, c, base, "pairs_device_indel_cross_product")
    ctx.close()


if __name__ == "__main__":
    main()
