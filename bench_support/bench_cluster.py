#!/usr/bin/env python3
"""Cluster (strsim_cluster_device) timing, one JSON line per case, device-resident.

Every call is timed with hipEvents recorded on the context's stream around it (median of 10 timed repetitions behind 3 warm-ups;
the minimum and maximum of the 10 are reported beside every median).
Frame: the self-join of DESIGN.md section 21 -- near_duplicates(11, cands, 200 000) over cfg2's candidates -- by ratio at 0.9, and
the same by jaro_winkler.
Lines, per measure:
  - strsim_cluster_device as a whole (the join into the context's own buffer, then the components);
  - strsim_join_device / strsim_match_join_device with STRSIM_JOIN_UPPER at exact capacity on the same frame in the same process,
    alternated with the cluster call repetition by repetition;
  - strsim_components_device alone on that join's CSR, with edges per second;
  - strsim_join_host (ratio only): the only route before this call existed -- the pairs have to reach the host before any
    clustering can start.
Condition, on the ratio line: cluster_ms <= join_host_ms, with a gap larger than the max - min spread of
either call's 10 repetitions.
Reported, not conditioned: cluster_ms - join_device_ms (the price of the labels), the components call alone on a 5 000-leaf star,
and scipy.sparse.csgraph.connected_components on the host copy of the CSR where scipy is importable.

    python bench_support/bench_cluster.py [--out FILE] [--rows N]      (lines are appended to FILE, default
                                                                          profiles/cluster_bench_lines.jsonl)
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import strsim_amd as S
from strsim_amd._lib import check, lib
from bench_support.bench_extract import emit
from bench_support.bench_nearest import DEV, cfg2_column, host_column, near_duplicates, to_strings

WARMUP, REPS = 3, 10
UPPER = 1


def timed_alternately(ctx, calls):
    """the calls in turn, repetition by repetition -> one list of REPS milliseconds per call"""
    stream = torch.cuda.ExternalStream(ctx.stream, device=DEV)
    ms = [[] for _ in calls]
    for r in range(WARMUP + REPS):
        for k, call in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            ctx.synchronize()
            e1.synchronize()
            if r >= WARMUP:
                ms[k].append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    return round(float(np.median(ms)), 4), [round(min(ms), 4), round(max(ms), 4)]


def join_entry(measure):
    return "strsim_join" if measure == "ratio" else "strsim_match_join"


def measure_id(measure):
    return S.MEASURE_ID["indel" if measure == "ratio" else measure]


def bench_measure(ctx, f, measure, col, cutoff, host_strings):
    off, val = col
    n = off.numel() - 1
    mid = measure_id(measure)
    root = torch.empty(n, dtype=torch.int32, device=DEV)
    cluster = torch.empty(n, dtype=torch.int32, device=DEV)
    count, nnz = C.c_uint64(0), C.c_uint64(0)

    def cluster_call():
        check(lib().strsim_cluster_device(ctx._h, mid, off.data_ptr(), val.data_ptr(), n, cutoff, root.data_ptr(), cluster.data_ptr(),
                                          C.byref(count), C.byref(nnz)))
    cluster_call()
    ctx.synchronize()
    edges, clusters = nnz.value, count.value
    indptr = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    index = torch.empty(max(edges, 1), dtype=torch.int32, device=DEV)
    score = torch.empty(max(edges, 1), dtype=torch.float64, device=DEV)
    jn = C.c_uint64(0)
    join_device = getattr(lib(), join_entry(measure) + "_device")

    def join_call():
        check(join_device(ctx._h, mid, off.data_ptr(), val.data_ptr(), n, off.data_ptr(), val.data_ptr(), n, cutoff, UPPER, max(edges, 1),
                          indptr.data_ptr(), index.data_ptr(), score.data_ptr(), C.byref(jn)))
    ms_cluster, ms_join = timed_alternately(ctx, [cluster_call, join_call])
    assert jn.value == edges
    root2 = torch.empty_like(root)

    def components_call():
        check(lib().strsim_components_device(ctx._h, n, indptr.data_ptr(), index.data_ptr(), edges, root2.data_ptr(), cluster.data_ptr(), C.byref(count)))
    (ms_comp,) = timed_alternately(ctx, [components_call])
    assert count.value == clusters and torch.equal(root, root2)
    t_cluster, mm_cluster = stats(ms_cluster)
    t_join, mm_join = stats(ms_join)
    t_comp, mm_comp = stats(ms_comp)
    line = {"bench": "cluster", "measure": measure, "rows": n, "min_score": cutoff, "nnz": edges, "clusters": clusters, "cluster_ms": t_cluster,
            "cluster_min_max_ms": mm_cluster, "join_device_ms": t_join, "join_device_min_max_ms": mm_join,
            "labels_price_ms": round(t_cluster - t_join, 4), "components_ms": t_comp, "components_min_max_ms": mm_comp,
            "components_edges_per_s": round(edges / (t_comp / 1e3), 1) if t_comp else None}
    if host_strings is not None:
        ho, hv = S.pack_strings(host_strings)
        h_indptr = np.empty(n + 1, dtype=np.uint64)
        h_index, h_score = np.empty(max(edges, 1), dtype=np.uint32), np.empty(max(edges, 1), dtype=np.float64)
        join_host = getattr(lib(), join_entry(measure) + "_host")

        def host_call():
            check(join_host(ctx._h, mid, ho.ctypes.data, hv.ctypes.data, n, ho.ctypes.data, hv.ctypes.data, n, cutoff, UPPER, max(edges, 1),
                            h_indptr.ctypes.data, h_index.ctypes.data, h_score.ctypes.data, C.byref(jn)))
        (ms_host,) = timed_alternately(ctx, [host_call])
        t_host, mm_host = stats(ms_host)
        gap = t_host - t_cluster
        spread = max(mm_cluster[1] - mm_cluster[0], mm_host[1] - mm_host[0])
        line.update({"join_host_ms": t_host, "join_host_min_max_ms": mm_host, "condition": "cluster_ms <= join_host_ms, gap > spread",
                     "gap_ms": round(gap, 4), "spread_ms": round(spread, 4), "condition_met": bool(gap >= 0 and gap > spread)})
        try:
            from scipy.sparse import csr_matrix
            from scipy.sparse.csgraph import connected_components
            t0 = time.perf_counter()
            g = csr_matrix((np.ones(edges, dtype=np.int8), h_index[:edges].astype(np.int32), h_indptr.astype(np.int64)), shape=(n, n))
            ncomp, _ = connected_components(g, directed=False)
            line["scipy_connected_components_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
            assert ncomp == clusters
        except ImportError:
            pass
    emit(f, line)


def bench_star(ctx, f, leaves=5000):
    n = leaves + 1
    indptr = torch.arange(0, n + 1, dtype=torch.int64).clamp_(max=leaves).to(DEV)  # row v < leaves holds one edge, the centre none
    index = torch.full((leaves,), leaves, dtype=torch.int32).to(DEV)
    root = torch.empty(n, dtype=torch.int32, device=DEV)
    cluster = torch.empty(n, dtype=torch.int32, device=DEV)
    count = C.c_uint64(0)

    def call():
        check(lib().strsim_components_device(ctx._h, n, indptr.data_ptr(), index.data_ptr(), leaves, root.data_ptr(), cluster.data_ptr(), C.byref(count)))
    (ms,) = timed_alternately(ctx, [call])
    assert count.value == 1 and not root.any()
    t, mm = stats(ms)
    emit(f, {"bench": "components_star", "leaves": leaves, "components_ms": t, "components_min_max_ms": mm,
             "components_edges_per_s": round(leaves / (t / 1e3), 1)})


def main():
    args = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "cluster_bench_lines.jsonl"), "--rows": "200000"}
    while args:
        opt[args[0]] = args[1]
        args = args[2:]
    rows = int(opt["--rows"])
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = S.Context(0, stream=st.cuda_stream)
    cands = to_strings(cfg2_column(10000, 200_000))
    strings = near_duplicates(11, cands, rows)
    col = host_column(strings)
    torch.cuda.synchronize()
    with open(opt["--out"], "a") as f:
        bench_measure(ctx, f, "ratio", col, 0.9, strings)
        bench_measure(ctx, f, "jaro_winkler", col, 0.9, None)
        bench_star(ctx, f)
    ctx.close()


if __name__ == "__main__":
    main()
