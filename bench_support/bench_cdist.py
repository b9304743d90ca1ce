#!/usr/bin/env python3
"""cdist (strsim_cdist_device) timing, one JSON line per measure, device-resident.

Every call is timed with hipEvents recorded on the context's stream around it (median of 10 timed repetitions behind 3 warm-ups).
Frame: 20 000 queries x 10 000 candidates of cfg2's generator (U{1..32} ASCII), measures levenshtein, jaro_winkler and indel.
Beside each, in the same process on the same frame:
  (i)   the search with k = 1 (strsim_best_match_device; strsim_extract_device for indel): the same scores without the stores;
  (ii)  hipMemsetAsync of the same 1.6 GB matrix: what writing it costs on this device;
  (iii) the exploded pairwise call (strsim_pairs_device) on a slice of 2 000 queries (2 * 10^7 pairs), and cdist on that slice.
Condition: cdist_ms <= 1.25 * (search_ms + memset_ms).  The ratio to (iii) is reported only.  `tj` and
`block` label the line with the tile width and workgroup size the library was built with (STRSIM_CDIST_TJ, STRSIM_CDIST_BLOCK; run
once per build, STRSIM_AMD_LIB names the build).

    python bench_support/bench_cdist.py [--out FILE] [--tj N] [--block N] [--queries N] [--candidates N]
                                          (lines are appended to FILE, default profiles/cdist_bench_lines.jsonl)
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
from bench_support.bench_extract import cross_product, emit, extract_ms, timed
from bench_support.bench_nearest import DEV, cfg2_column, host_column, to_strings

MEASURES = ("levenshtein", "jaro_winkler", "indel")
MARGIN = 1.25


def cdist_ms(ctx, measure, q, c, out):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1

    def call():
        check(lib().strsim_cdist_device(ctx._h, measure, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc,
                                        float("-inf"), out.data_ptr(), nc))
    return timed(ctx, call)


def memset_ms(ctx, out):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.restype = C.c_int
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    nbytes = out.numel() * 8

    def call():
        assert hip.hipMemsetAsync(out.data_ptr(), 0, nbytes, ctx.stream) == 0
    return timed(ctx, call)


def main():
    args = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "cdist_bench_lines.jsonl"), "--tj": "8", "--block": "512", "--queries": "20000", "--candidates": "10000"}
    while args:
        opt[args[0]] = args[1]
        args = args[2:]
    nq, nc, slice_q = int(opt["--queries"]), int(opt["--candidates"]), 2_000
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = S.Context(0, stream=st.cuda_stream)
    q, c = cfg2_column(nq, 0), cfg2_column(nc, 200_000)
    qs = host_column(to_strings(q)[:slice_q])
    out = torch.empty((nq, nc), dtype=torch.float64, device=DEV)
    (ao, av), (bo, bv) = cross_product(qs, c)
    n = ao.numel() - 1
    res = torch.empty(n, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    ms_set = memset_ms(ctx, out)
    with open(opt["--out"], "a") as f:
        for name in MEASURES:
            m = S.MEASURE_ID[name]
            t = cdist_ms(ctx, m, q, c, out)
            search = extract_ms(ctx, m, q, c, 1, None) if name == "indel" else best_match_ms_of(ctx, m, q, c)
            t_slice = cdist_ms(ctx, m, qs, c, out)

            def pairs():
                check(lib().strsim_pairs_device(ctx._h, m, ao.data_ptr(), av.data_ptr(), n, bo.data_ptr(), bv.data_ptr(), n, res.data_ptr(), n))
            t_pairs = timed(ctx, pairs)
            bound = MARGIN * (search + ms_set)
            emit(f, {"bench": "cdist", "measure": name, "tj": int(opt["--tj"]), "block": int(opt["--block"]), "queries": nq, "candidates": nc, "cdist_ms": round(t, 4),
                     "pairs_per_s": round(nq * nc / (t / 1e3), 1), "matrix_gb_per_s": round(nq * nc * 8 / (t / 1e3) / 1e9, 1),
                     "search_k1": "extract" if name == "indel" else "best_match", "search_k1_ms": round(search, 4),
                     "memset_ms": round(ms_set, 4), "bound_ms": round(bound, 4), "condition_met": bool(t <= bound),
                     "slice_pairs": n, "slice_cdist_ms": round(t_slice, 4), "slice_pairwise_ms": round(t_pairs, 4),
                     "slice_pairwise_over_cdist": round(t_pairs / t_slice, 2)})
    ctx.close()


def best_match_ms_of(ctx, measure, q, c):
    """bench_extract.best_match_ms at a measure of one's choice"""
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    idx = torch.empty((nq, 1), dtype=torch.int32, device=DEV)
    sc = torch.empty((nq, 1), dtype=torch.float64, device=DEV)

    def bm():
        check(lib().strsim_best_match_device(ctx._h, measure, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc,
                                             1, float("-inf"), idx.data_ptr(), sc.data_ptr()))
    return timed(ctx, bm)


if __name__ == "__main__":
    main()
