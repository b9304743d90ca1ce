#!/usr/bin/env python3
"""match_join (strsim_match_join_device) timing, one JSON line per case, device-resident.

bench_join.py's frame and method: 10 000 candidates of cfg2's generator (U{1..32} ASCII) and 20 000 queries that are a random
candidate with 0 .. 3 random edits; every call is timed with hipEvents recorded on the context's stream around it, median of 10
timed repetitions behind 3 warm-ups; the whole join is one call -- both sweeps, the scan, the nnz wait, the fill and the sort --
with capacity = the exact nnz, found by a count-only call outside the timed region.
The yardstick is strsim_cdist_device(measure, the same cutoff) on the same frame in the same process, today's only other route to
the same answer (it still leaves a 1.6 GB matrix to compact); the two calls are ALTERNATED, repetition by repetition, and the
spread of each (min and max of the 10) is reported beside its median.
Condition: for levenshtein, jaccard and sorensen_dice at min_score 0.8, match_join_ms <= cdist_ms.
Reported beside it, not conditioned: jaro and jaro_winkler at 0.8 and 0.9, the count-only call, nnz, `mask_pairs` (the pairs the
need mask admits, waves of 64 queries in length order) and (--self N, default 200 000; 0 skips it) an `upper` self-join of N near
duplicates at 0.9 by levenshtein and jaro_winkler; and, because the frame's 0.8 % of 33-byte queries go through one pairwise call
each in match_join and cdist alike and dominate both, the lines of frame "lane_class_only": the same queries cut to 32 bytes, where
the two calls are their sweeps.

    python bench_support/bench_match_join.py [--out FILE] [--queries N] [--candidates N] [--self N]
                                         (lines are appended to FILE, default profiles/match_join_bench_lines.jsonl)
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import strsim_amd as S
from strsim_amd._lib import check, lib
from bench_support.bench_extract import byte_lengths, emit
from bench_support.bench_nearest import DEV, cfg2_column, host_column, near_duplicates, to_strings

CASES = (("levenshtein", 0.8, True), ("jaccard", 0.8, True), ("sorensen_dice", 0.8, True), ("jaro", 0.8, False), ("jaro", 0.9, False),
         ("jaro_winkler", 0.8, False), ("jaro_winkler", 0.9, False))
WARMUP, REPS = 3, 10


def ub(measure, lq, lc):
    """match_join_ub of strsim_match_join.h restated in Python doubles (the same IEEE operations in the same order)"""
    if lq == 0 and lc == 0:
        return 1.0
    if lq == 0 or lc == 0:
        return 0.0
    mn = float(min(lq, lc))
    if measure == "levenshtein":
        return 1.0 - (float(abs(lq - lc)) / float(max(lq, lc)))
    if measure in ("jaro", "jaro_winkler"):
        j = (mn / float(lq) + mn / float(lc) + mn / mn) / 3.0
        return j + (min(4.0, mn) * 0.1 * (1.0 - j)) if measure == "jaro_winkler" and j > 0.7 else j
    if measure == "jaccard":
        return mn / float(lq + lc - min(lq, lc))
    return 2.0 * mn / float(lq + lc)


def mask_pairs(measure, q, c, cutoff):
    """pairs the need mask admits: a wave of 64 queries (length order) visits a length iff one of its queries needs it"""
    lq, lc = np.sort(byte_lengths(q)), byte_lengths(c)
    lq = lq[lq <= 32]
    hist = np.bincount(lc[lc <= 32], minlength=33)
    need = np.array([[ub(measure, a, b) >= cutoff for b in range(33)] for a in range(33)])
    total = 0
    for w0 in range(0, lq.size, 64):
        wave = lq[w0:w0 + 64]
        total += wave.size * int(hist[need[np.unique(wave)].any(axis=0)].sum())
    return total


def event_ms(ctx, stream, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    ctx.synchronize()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternated(ctx, calls):
    """every call of `calls` in turn, WARMUP + REPS rounds -> per call (median, min, max) of the timed rounds"""
    stream = torch.cuda.ExternalStream(ctx.stream, device=DEV)
    ms = [[] for _ in calls]
    for r in range(WARMUP + REPS):
        for k, call in enumerate(calls):
            t = event_ms(ctx, stream, call)
            if r >= WARMUP:
                ms[k].append(t)
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def join_call(ctx, mid, q, c, cutoff, flags, capacity, indptr, index, score):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    nnz = C.c_uint64(0)

    def call():
        check(lib().strsim_match_join_device(ctx._h, mid, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc, cutoff, flags,
                                             capacity, indptr.data_ptr(), index.data_ptr() if capacity else None,
                                             score.data_ptr() if capacity else None, C.byref(nnz)))
    return call, nnz


def cdist_call(ctx, mid, q, c, cutoff, out):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    return lambda: check(lib().strsim_cdist_device(ctx._h, mid, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc, cutoff,
                                                   out.data_ptr(), nc))


def prepared_join(ctx, mid, q, c, cutoff, flags=0):
    """-> (count-only call, whole-join call, nnz); the outputs stay alive with the closures"""
    nq = q[0].numel() - 1
    indptr = torch.empty(nq + 1, dtype=torch.int64, device=DEV)
    count, nnz = join_call(ctx, mid, q, c, cutoff, flags, 0, indptr, None, None)
    count()
    ctx.synchronize()
    n = nnz.value
    index = torch.empty(max(n, 1), dtype=torch.int32, device=DEV)
    score = torch.empty(max(n, 1), dtype=torch.float64, device=DEV)
    whole, nnz2 = join_call(ctx, mid, q, c, cutoff, flags, max(n, 1), indptr, index, score)
    whole()
    ctx.synchronize()
    assert nnz2.value == n
    return count, whole, n


def main():
    args = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "match_join_bench_lines.jsonl"), "--queries": "20000", "--candidates": "10000", "--self": "200000"}
    while args:
        opt[args[0]] = args[1]
        args = args[2:]
    nq, nc, nself = int(opt["--queries"]), int(opt["--candidates"]), int(opt["--self"])
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = S.Context(0, stream=st.cuda_stream)
    c = cfg2_column(nc, 200_000)
    cands = to_strings(c)
    queries = near_duplicates(7, cands, nq)
    q = host_column(queries)
    q32 = host_column([s[:32] for s in queries])
    out = torch.empty((nq, nc), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    with open(opt["--out"], "a") as f:
        for frame, q, measure, cutoff, conditioned in [("bench_join", q, *case) for case in CASES] + [("lane_class_only", q32, *case[:2], False)
                                                                                                     for case in CASES]:
            mid = S.MEASURE_ID[measure]
            count, whole, nnz = prepared_join(ctx, mid, q, c, cutoff)
            (t, t_lo, t_hi), (t_cdist, c_lo, c_hi), (t_count, _, _) = alternated(ctx, [whole, cdist_call(ctx, mid, q, c, cutoff, out), count])
            mp = mask_pairs(measure, q, c, cutoff)
            line = {"bench": "match_join", "frame": frame, "measure": measure, "queries": nq, "candidates": nc, "min_score": cutoff, "nnz": nnz,
                    "match_join_ms": round(t, 4), "match_join_min_max_ms": [round(t_lo, 4), round(t_hi, 4)], "count_only_ms": round(t_count, 4),
                    "pairs_per_s": round(nq * nc / (t / 1e3), 1), "cdist_same_cutoff_ms": round(t_cdist, 4),
                    "cdist_min_max_ms": [round(c_lo, 4), round(c_hi, 4)], "mask_pairs": mp, "mask_fraction": round(mp / (nq * nc), 4)}
            if conditioned:
                line["condition"] = "match_join_ms <= cdist_same_cutoff_ms"
                line["condition_met"] = bool(t <= t_cdist)
            emit(f, line)
        del out
        if nself:
            x = host_column(near_duplicates(11, cands, nself))
            for measure in ("levenshtein", "jaro_winkler"):
                count, whole, nnz = prepared_join(ctx, S.MEASURE_ID[measure], x, x, 0.9, 1)
                (t, t_lo, t_hi), (t_count, _, _) = alternated(ctx, [whole, count])
                emit(f, {"bench": "match_join_self_upper", "measure": measure, "rows": nself, "min_score": 0.9, "nnz": nnz, "match_join_ms": round(t, 4),
                         "match_join_min_max_ms": [round(t_lo, 4), round(t_hi, 4)], "count_only_ms": round(t_count, 4),
                         "pairs_per_s": round(nself * nself / (t / 1e3), 1)})
    ctx.close()


if __name__ == "__main__":
    main()
