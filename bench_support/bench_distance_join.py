#!/usr/bin/env python3
"""distance_join (strsim_distance_join_device) timing, one JSON line per case, device-resident.

bench_match_join.py's frames and method: 10 000 candidates of cfg2's generator (U{1..32} ASCII) and 20 000 queries that are a random
candidate with 0 .. 3 random edits (frame "bench_join"; "lane_class_only": the same queries cut to 32 bytes, where a call is its
sweeps); every call is timed with hipEvents recorded on the context's stream around it, median of 10 timed repetitions behind 3
warm-ups, min and max beside it; the whole join is one call -- both sweeps, the scan, the nnz wait, the fill, the sort and the
finishing kernel -- with capacity = the exact nnz, found by a count-only call outside the timed region.

Condition, on lane_class_only, the calls ALTERNATED repetition by repetition in one process:
    distance_join("levenshtein", 2) <= match_join("levenshtein", 0.8)   and   distance_join("osa", 2) <= match_join("levenshtein", 0.8)
Reported beside it, not conditioned (--section main): every kind at k = 0 .. 3 on both frames with the count-only call; the share
of the visited candidates whose wave ran the Damerau-Levenshtein cell DP, computed on the host from the OSA join at 2 k (waves of 64
queries in stable length order, an estimate of the kernel's own order inside a length); the pairwise
damerau_levenshtein_distance call over the explicit window pairs of the first 2 000 queries beside the join of those queries.
--section self: the `upper` self-join of N near duplicates (default 200 000) at k = 2 by all three kinds, and distance_cluster on
the same frame.

    python bench_support/bench_distance_join.py [--out FILE] [--section main|self] [--queries N] [--candidates N] [--self N]
                                            (lines are appended to FILE, default profiles/distance_join_bench_lines.jsonl)
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
from bench_support.bench_extract import emit
from bench_support.bench_match_join import alternated, prepared_join
from bench_support.bench_nearest import DEV, byte_lengths, cfg2_column, host_column, near_duplicates, to_strings

KINDS = S.DISTANCE_JOIN_MEASURES
UNBOUNDED = 0xFFFFFFFF


def join_call(ctx, kind, q, c, k, flags, capacity, indptr, index, dist):
    qoff, qval = q
    coff, cval = c
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    nnz = C.c_uint64(0)

    def call():
        check(lib().strsim_distance_join_device(ctx._h, kind, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc, k, flags,
                                                capacity, indptr.data_ptr(), index.data_ptr() if capacity else None,
                                                dist.data_ptr() if capacity else None, C.byref(nnz)))
    return call, nnz


def prepared(ctx, kind, q, c, k, flags=0):
    """-> (count-only call, whole-join call, nnz, (indptr, index, dist)); the outputs stay alive with the closures"""
    nq = q[0].numel() - 1
    indptr = torch.empty(nq + 1, dtype=torch.int64, device=DEV)
    count, nnz = join_call(ctx, kind, q, c, k, flags, 0, indptr, None, None)
    count()
    ctx.synchronize()
    n = nnz.value
    index = torch.empty(max(n, 1), dtype=torch.int32, device=DEV)
    dist = torch.empty(max(n, 1), dtype=torch.int32, device=DEV)
    whole, nnz2 = join_call(ctx, kind, q, c, k, flags, max(n, 1), indptr, index, dist)
    whole()
    ctx.synchronize()
    assert nnz2.value == n
    return count, whole, n, (indptr, index, dist)


def window_fraction(q, c, k):
    """the share of all pairs that a wave of 64 queries (stable length order) visits: a length within k of one of its queries'"""
    lq, lc = np.sort(byte_lengths(q), kind="stable"), byte_lengths(c)
    lq = lq[lq <= 32]
    hist = np.bincount(lc[lc <= 32], minlength=33)
    total = 0
    for w0 in range(0, lq.size, 64):
        wave = np.unique(lq[w0:w0 + 64])
        lens = np.arange(33)
        total += (lq[w0:w0 + 64].size) * int(hist[(np.abs(lens[None, :] - wave[:, None]) <= k).any(axis=0)].sum())
    return total / float(byte_lengths(q).size * lc.size)


def dp_share(ctx, q, c, k):
    """(wave, candidate) visits whose wave has an undecided lane / all (wave, candidate) visits, from the OSA join at 2 k"""
    _, _, n, (indptr, index, dist) = prepared(ctx, 1, q, c, 2 * k)
    ip, ix, o = indptr.cpu().numpy(), index.cpu().numpy()[:n].astype(np.int64), dist.cpu().numpy()[:n].astype(np.int64)
    lq, lc = byte_lengths(q), byte_lengths(c)
    rows = np.repeat(np.arange(lq.size), np.diff(ip))
    und = (o >= 3) & (o <= 2 * k) & (np.abs(lq[rows] - lc[ix]) <= k) & (lq[rows] <= 32) & (lc[ix] <= 32)
    fast = np.flatnonzero(lq <= 32)
    order = fast[np.argsort(lq[fast], kind="stable")]
    wave_of = np.full(lq.size, -1, dtype=np.int64)
    wave_of[order] = np.arange(order.size) // 64
    ran = np.unique(wave_of[rows[und]] * lc.size + ix[und]).size
    hist = np.bincount(lc[lc <= 32], minlength=33)
    lens = np.arange(33)
    visits = 0
    for w0 in range(0, order.size, 64):
        wave = np.unique(lq[order[w0:w0 + 64]])
        visits += int(hist[(np.abs(lens[None, :] - wave[:, None]) <= k).any(axis=0)].sum())
    return ran / float(visits), int(und.sum())


def main():
    args = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "distance_join_bench_lines.jsonl"), "--section": "main", "--queries": "20000",
           "--candidates": "10000", "--self": "200000"}
    while args:
        opt[args[0]] = args[1]
        args = args[2:]
    nq, nc, nself = int(opt["--queries"]), int(opt["--candidates"]), int(opt["--self"])
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = S.Context(0, stream=st.cuda_stream)
    c = cfg2_column(nc, 200_000)
    cands = to_strings(c)
    with open(opt["--out"], "a") as f:
        if opt["--section"] == "main":
            queries = near_duplicates(7, cands, nq)
            frames = (("bench_join", host_column(queries)), ("lane_class_only", host_column([s[:32] for s in queries])))
            torch.cuda.synchronize()
            # the condition: alternated with match_join("levenshtein", 0.8) on lane_class_only
            q = frames[1][1]
            _, lev, n_lev, keep1 = prepared(ctx, 0, q, c, 2)
            _, osa, n_osa, keep2 = prepared(ctx, 1, q, c, 2)
            _, mj, n_mj = prepared_join(ctx, S.MEASURE_ID["levenshtein"], q, c, 0.8)
            (t_lev, lev_lo, lev_hi), (t_osa, osa_lo, osa_hi), (t_mj, mj_lo, mj_hi) = alternated(ctx, [lev, osa, mj])
            for kind, t, lo, hi, n in (("levenshtein", t_lev, lev_lo, lev_hi, n_lev), ("osa", t_osa, osa_lo, osa_hi, n_osa)):
                emit(f, {"bench": "distance_join_condition", "frame": "lane_class_only", "measure": kind, "queries": nq, "candidates": nc,
                         "max_distance": 2, "nnz": n, "distance_join_ms": round(t, 4), "distance_join_min_max_ms": [round(lo, 4), round(hi, 4)],
                         "match_join_levenshtein_0.8_ms": round(t_mj, 4), "match_join_min_max_ms": [round(mj_lo, 4), round(mj_hi, 4)],
                         "match_join_nnz": n_mj, "window_fraction": round(window_fraction(q, c, 2), 4),
                         "condition": "distance_join_ms <= match_join_levenshtein_0.8_ms", "condition_met": bool(t <= t_mj)})
            del keep1, keep2
            # every kind at k = 0 .. 3, whole call and count-only
            for frame, q in frames:
                for k in (0, 1, 2, 3):
                    calls, nnzs = [], []
                    for kind in range(3):
                        count, whole, n, keep = prepared(ctx, kind, q, c, k)
                        calls += [whole, count]
                        nnzs.append((n, keep))
                    ms = alternated(ctx, calls)
                    share = dp_share(ctx, q, c, k) if k >= 1 else (0.0, 0)
                    for kind in range(3):
                        (t, lo, hi), (t_count, _, _) = ms[2 * kind], ms[2 * kind + 1]
                        line = {"bench": "distance_join", "frame": frame, "measure": KINDS[kind], "queries": nq, "candidates": nc, "max_distance": k,
                                "nnz": nnzs[kind][0], "distance_join_ms": round(t, 4), "distance_join_min_max_ms": [round(lo, 4), round(hi, 4)],
                                "count_only_ms": round(t_count, 4), "pairs_per_s": round(nq * nc / (t / 1e3), 1),
                                "window_fraction": round(window_fraction(q, c, k), 4)}
                        if kind == 2:
                            line["osa_same_k_ms"] = round(ms[2][0], 4)
                            line["dp_share_of_visits"] = round(share[0], 6)
                            line["undecided_pairs"] = share[1]
                        emit(f, line)
            # the pairwise call over the explicit window pairs of the first 2 000 queries
            sub = [s[:32] for s in queries[:2000]]
            lq, lc = np.array([len(s.encode()) for s in sub]), np.array([len(s.encode()) for s in cands])
            qsub = host_column(sub)
            for k in (1, 2, 3):
                i, j = np.nonzero(np.abs(lq[:, None] - lc[None, :]) <= k)
                a, b = host_column([sub[x] for x in i]), host_column([cands[x] for x in j])
                out = torch.empty(i.size, dtype=torch.int32, device=DEV)
                pair = lambda: check(lib().strsim_damerau_distance_device(ctx._h, a[0].data_ptr(), a[1].data_ptr(), i.size, b[0].data_ptr(),
                                                                          b[1].data_ptr(), i.size, k, out.data_ptr(), i.size))
                _, whole, n, keep = prepared(ctx, 2, qsub, c, k)
                (t, lo, hi), (t_pair, p_lo, p_hi) = alternated(ctx, [whole, pair])
                ctx.synchronize()
                assert int((out.cpu().numpy() <= k).sum()) == n
                emit(f, {"bench": "distance_join_vs_pairwise", "measure": "damerau_levenshtein", "queries": len(sub), "candidates": nc,
                         "max_distance": k, "window_pairs": int(i.size), "nnz": n, "distance_join_ms": round(t, 4),
                         "distance_join_min_max_ms": [round(lo, 4), round(hi, 4)], "pairwise_window_pairs_ms": round(t_pair, 4),
                         "pairwise_min_max_ms": [round(p_lo, 4), round(p_hi, 4)]})
                del a, b, out
        else:
            x = host_column(near_duplicates(11, cands, nself))
            torch.cuda.synchronize()
            for kind in range(3):
                count, whole, nnz, keep = prepared(ctx, kind, x, x, 2, 1)
                root = torch.empty(nself, dtype=torch.int32, device=DEV)
                label = torch.empty(nself, dtype=torch.int32, device=DEV)
                cnt, pairs = C.c_uint64(0), C.c_uint64(0)
                cluster = lambda: check(lib().strsim_distance_cluster_device(ctx._h, kind, x[0].data_ptr(), x[1].data_ptr(), nself, 2, root.data_ptr(),
                                                                             label.data_ptr(), C.byref(cnt), C.byref(pairs)))
                (t, t_lo, t_hi), (t_count, _, _), (t_cl, cl_lo, cl_hi) = alternated(ctx, [whole, count, cluster])
                assert pairs.value == nnz
                emit(f, {"bench": "distance_join_self_upper", "measure": KINDS[kind], "rows": nself, "max_distance": 2, "nnz": nnz,
                         "distance_join_ms": round(t, 4), "distance_join_min_max_ms": [round(t_lo, 4), round(t_hi, 4)],
                         "count_only_ms": round(t_count, 4), "pairs_per_s": round(nself * nself / (t / 1e3), 1), "clusters": cnt.value,
                         "distance_cluster_ms": round(t_cl, 4), "distance_cluster_min_max_ms": [round(cl_lo, 4), round(cl_hi, 4)]})
    ctx.close()


if __name__ == "__main__":
    main()
