#!/usr/bin/env python3
"""Threshold join (strsim_join_device) timing, one JSON line per case, device-resident.

Every call is timed with hipEvents recorded on the context's stream around it (median of 10 timed repetitions behind 3 warm-ups).
Frame: bench_extract's frame (b) cut to cdist's size -- 10 000 candidates of cfg2's generator (U{1..32} ASCII) and 20 000 queries
that are a random candidate with 0 .. 3 random edits -- scorer ratio.  The whole join is one call: both sweeps, the scan, the nnz
wait, the fill and the sort (capacity = the exact nnz, found by a count-only call outside the timed region).
Condition: at cutoff 0.8, join_ms <= cdist_ms, strsim_cdist_device(STRSIM_INDEL, the same cutoff) on the same
frame in the same process -- today's only way to the same answer, which still leaves a 1.6 GB matrix to compact.  `window_pairs`
(bench_extract) is the number of pairs the static window admits.
Reported beside it, not conditioned: the same at 0.9, extract(k = 1, the same cutoff), the count-only call, and (--self N, default
200 000; 0 skips it) an `upper` self-join of N near duplicates at 0.9 with its pairs/s and nnz.

    python bench_support/bench_join.py [--out FILE] [--queries N] [--candidates N] [--self N]
                                         (lines are appended to FILE, default profiles/join_bench_lines.jsonl)
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import torch

import strsim_amd as S
from strsim_amd._lib import check, lib
from bench_support.bench_extract import emit, extract_ms, timed, window_pairs
from bench_support.bench_nearest import DEV, cfg2_column, host_column, near_duplicates, to_strings

INDEL = S.MEASURE_ID["indel"]


def join_call(ctx, q, c, cutoff, flags, capacity, indptr, index, score):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    nnz = C.c_uint64(0)

    def call():
        check(lib().strsim_join_device(ctx._h, INDEL, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc, cutoff, flags,
                                       capacity, indptr.data_ptr(), index.data_ptr() if capacity else None, score.data_ptr() if capacity else None,
                                       C.byref(nnz)))
    return call, nnz


def join_ms(ctx, q, c, cutoff, flags=0):
    """-> (whole join ms, count-only ms, nnz)"""
    nq = q[0].numel() - 1
    indptr = torch.empty(nq + 1, dtype=torch.int64, device=DEV)
    count, nnz = join_call(ctx, q, c, cutoff, flags, 0, indptr, None, None)
    t_count = timed(ctx, count)
    n = nnz.value
    index = torch.empty(max(n, 1), dtype=torch.int32, device=DEV)
    score = torch.empty(max(n, 1), dtype=torch.float64, device=DEV)
    whole, nnz2 = join_call(ctx, q, c, cutoff, flags, max(n, 1), indptr, index, score)
    t = timed(ctx, whole)
    assert nnz2.value == n
    return t, t_count, n


def cdist_ms(ctx, q, c, cutoff, out):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1

    def call():
        check(lib().strsim_cdist_device(ctx._h, INDEL, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc, cutoff,
                                        out.data_ptr(), nc))
    return timed(ctx, call)


def main():
    args = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "join_bench_lines.jsonl"), "--queries": "20000", "--candidates": "10000", "--self": "200000"}
    while args:
        opt[args[0]] = args[1]
        args = args[2:]
    nq, nc, nself = int(opt["--queries"]), int(opt["--candidates"]), int(opt["--self"])
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = S.Context(0, stream=st.cuda_stream)
    c = cfg2_column(nc, 200_000)
    cands = to_strings(c)
    q = host_column(near_duplicates(7, cands, nq))
    out = torch.empty((nq, nc), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    with open(opt["--out"], "a") as f:
        for cutoff, conditioned in ((0.8, True), (0.9, False)):
            t, t_count, nnz = join_ms(ctx, q, c, cutoff)
            t_cdist = cdist_ms(ctx, q, c, cutoff, out)
            t_extract = extract_ms(ctx, INDEL, q, c, 1, cutoff)
            wp = window_pairs(q, c, cutoff)
            line = {"bench": "join", "scorer": "ratio", "queries": nq, "candidates": nc, "cutoff": cutoff, "nnz": nnz, "join_ms": round(t, 4),
                    "count_only_ms": round(t_count, 4), "pairs_per_s": round(nq * nc / (t / 1e3), 1), "cdist_same_cutoff_ms": round(t_cdist, 4),
                    "extract_k1_ms": round(t_extract, 4), "window_pairs": wp, "window_fraction": round(wp / (nq * nc), 4)}
            if conditioned:
                line["condition"] = "join_ms <= cdist_same_cutoff_ms"
                line["condition_met"] = bool(t <= t_cdist)
            emit(f, line)
        del out
        if nself:
            x = host_column(near_duplicates(11, cands, nself))
            t, t_count, nnz = join_ms(ctx, x, x, 0.9, 1)
            emit(f, {"bench": "join_self_upper", "scorer": "ratio", "rows": nself, "cutoff": 0.9, "nnz": nnz, "join_ms": round(t, 4),
                     "count_only_ms": round(t_count, 4), "pairs_per_s": round(nself * nself / (t / 1e3), 1)})
    ctx.close()


if __name__ == "__main__":
    main()
