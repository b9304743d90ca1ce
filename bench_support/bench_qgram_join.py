#!/usr/bin/env python3
"""qgram_join (strsim_qgram_join_device) timing, one JSON line per case, device-resident.

bench_match_join.py's frame "lane_class_only" and method: 10 000 candidates of cfg2's generator (U{1..32} ASCII) and 20 000 queries
that are a random candidate with 0 .. 3 random edits, cut to 32 bytes; every call is timed with hipEvents recorded on the context's
stream around it, median of 10 timed repetitions behind 3 warm-ups, the calls of a case ALTERNATED repetition by repetition in one
process; the whole join is one call -- both sweeps, the scan, the nnz wait, the fill and the sort -- with capacity = the exact nnz,
found by a count-only call outside the timed region.
The yardstick is strsim_qgram_device over the same queries x candidates pairs laid out as two explicit device-resident pair columns
(built in slices of --slice queries outside the timed region; --queries 4000 where the memory does not allow 2 x 10^8 pairs).
Condition: for sorensen_dice, q = 2, multiset at min_score 0.8, qgram_join_ms <= pairwise_ms.  No margin.
Reported beside it, not conditioned: match_join("sorensen_dice", 0.8) on the same frame with the mask pairs of each, q = 3, set
mode, overlap (never pruned), the count-only call, and (--self N, default 200 000; 0 skips it) the `upper` self-join of N near
duplicates at 0.8.

    python bench_support/bench_qgram_join.py [--out FILE] [--queries N] [--candidates N] [--self N] [--slice N]
                                         (lines are appended to FILE, default profiles/qgram_join_bench_lines.jsonl)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import strsim_amd as S
from strsim_amd._lib import check, lib, qgram_args
from bench_support.bench_best_match import cross_slice
from bench_support.bench_extract import byte_lengths, emit
from bench_support.bench_match_join import alternated, mask_pairs as match_mask_pairs, prepared_join as prepared_match_join
from bench_support.bench_nearest import DEV, cfg2_column, host_column, near_duplicates, to_strings

# kind, q, multiset, min_score, conditioned
CASES = (("sorensen_dice", 2, True, 0.8, True), ("sorensen_dice", 3, True, 0.8, False), ("sorensen_dice", 2, False, 0.8, False),
         ("overlap", 2, True, 0.8, False), ("jaccard", 3, False, 0.8, False))


_HARNESS = None


def need_mask(kind, q, multiset, cutoff):
    """the 33 x 33 need relation of a call, from the library's own qgram_join_need_mask: strsim_qgram_join.h compiled by g++ through
    the host harness of the tests, never a restatement of the bound"""
    global _HARNESS
    if _HARNESS is None:
        so = os.path.join(tempfile.mkdtemp(prefix="qgram_join_harness_"), "libqgram_join_harness.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-fPIC", "-shared", "-I", os.path.join(ROOT, "polars-strsim_amd", "csrc"), "-o", so,
                               os.path.join(ROOT, "tests", "cpu_harness", "qgram_join_harness.cpp")])
        _HARNESS = C.CDLL(so)
        _HARNESS.qj_need_mask.restype = C.c_int
        _HARNESS.qj_need_mask.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_double, C.POINTER(C.c_uint64)]
    w = (C.c_uint64 * 33)()
    _HARNESS.qj_need_mask(S.QGRAM_KINDS.index(kind), q, 0 if multiset else 1, cutoff, w)
    return np.array([[(w[a] >> b) & 1 for b in range(33)] for a in range(33)], dtype=bool)


def mask_pairs(kind, q, multiset, qcol, ccol, cutoff):
    """pairs the need mask admits: a wave of 64 queries (length order) visits a length iff one of its queries needs it"""
    lq, lc = np.sort(byte_lengths(qcol)), byte_lengths(ccol)
    lq = lq[lq <= 32]
    hist = np.bincount(lc[lc <= 32], minlength=33)
    need = need_mask(kind, q, multiset, cutoff)
    total = 0
    for w0 in range(0, lq.size, 64):
        wave = lq[w0:w0 + 64]
        total += wave.size * int(hist[need[np.unique(wave)].any(axis=0)].sum())
    return total


def join_call(ctx, mode, qcol, ccol, cutoff, flags, capacity, indptr, index, score):
    (qoff, qval), (coff, cval) = qcol, ccol
    nq, nc = qoff.numel() - 1, coff.numel() - 1
    nnz = C.c_uint64(0)

    def call():
        check(lib().strsim_qgram_join_device(ctx._h, *mode, qoff.data_ptr(), qval.data_ptr(), nq, coff.data_ptr(), cval.data_ptr(), nc, cutoff, flags,
                                             capacity, indptr.data_ptr(), index.data_ptr() if capacity else None,
                                             score.data_ptr() if capacity else None, C.byref(nnz)))
    return call, nnz


def prepared_join(ctx, mode, qcol, ccol, cutoff, flags=0):
    """-> (count-only call, whole-join call, nnz); the outputs stay alive with the closures"""
    nq = qcol[0].numel() - 1
    indptr = torch.empty(nq + 1, dtype=torch.int64, device=DEV)
    count, nnz = join_call(ctx, mode, qcol, ccol, cutoff, flags, 0, indptr, None, None)
    count()
    ctx.synchronize()
    n = nnz.value
    index = torch.empty(max(n, 1), dtype=torch.int32, device=DEV)
    score = torch.empty(max(n, 1), dtype=torch.float64, device=DEV)
    whole, nnz2 = join_call(ctx, mode, qcol, ccol, cutoff, flags, max(n, 1), indptr, index, score)
    whole()
    ctx.synchronize()
    assert nnz2.value == n
    return count, whole, n


def pair_columns(qcol, ccol, step):
    """every (query, candidate) pair as two explicit pair columns, built `step` queries at a time"""
    (qoff, qval), (coff, cval) = qcol, ccol
    nq = qoff.numel() - 1
    offs, vals, base = ([], []), ([], []), [0, 0]
    for r0 in range(0, nq, step):
        n = min(step, nq - r0)
        part = cross_slice(qoff[r0:], qval, coff, cval, n)
        for side, (o, v) in enumerate(part):
            o64 = o.to(torch.int64) & 0xFFFFFFFF
            offs[side].append(o64[:-1] + base[side])
            vals[side].append(v[:-64])
            base[side] += int(o64[-1].item())
    assert max(base) < 2 ** 32, "the pair columns need 32-bit offsets: fewer queries"
    cols = []
    for side in range(2):
        o = torch.cat(offs[side] + [torch.tensor([base[side]], dtype=torch.int64, device=DEV)])
        cols.append((o.to(torch.int32), torch.cat(vals[side] + [torch.zeros(64, dtype=torch.uint8, device=DEV)])))
    return cols


def main():
    args = sys.argv[1:]
    opt = {"--out": os.path.join(ROOT, "profiles", "qgram_join_bench_lines.jsonl"), "--queries": "20000", "--candidates": "10000", "--self": "200000",
           "--slice": "1000"}
    while args:
        opt[args[0]] = args[1]
        args = args[2:]
    nq, nc, nself = int(opt["--queries"]), int(opt["--candidates"]), int(opt["--self"])
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = S.Context(0, stream=st.cuda_stream)
    c = cfg2_column(nc, 200_000)
    cands = to_strings(c)
    q = host_column([s[:32] for s in near_duplicates(7, cands, nq)])
    pa, pb = pair_columns(q, c, int(opt["--slice"]))
    pairs = nq * nc
    assert pa[0].numel() - 1 == pairs
    pout = torch.empty(pairs, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    with open(opt["--out"], "a") as f:
        for kind, qq, multiset, cutoff, conditioned in CASES:
            mode = qgram_args(kind, qq, multiset)
            count, whole, nnz = prepared_join(ctx, mode, q, c, cutoff)
            pairwise = lambda: check(lib().strsim_qgram_device(ctx._h, *mode, pa[0].data_ptr(), pa[1].data_ptr(), pairs, pb[0].data_ptr(),
                                                              pb[1].data_ptr(), pairs, pout.data_ptr(), pairs))
            (t, t_lo, t_hi), (t_pair, p_lo, p_hi), (t_count, _, _) = alternated(ctx, [whole, pairwise, count])
            # the join's hits are the pairwise call's scores at or above the cutoff
            assert int((pout >= cutoff).sum().item()) == nnz
            mp = mask_pairs(kind, qq, multiset, q, c, cutoff)
            line = {"bench": "qgram_join", "frame": "lane_class_only", "kind": kind, "q": qq, "multiset": multiset, "queries": nq, "candidates": nc,
                    "min_score": cutoff, "nnz": nnz, "qgram_join_ms": round(t, 4), "qgram_join_min_max_ms": [round(t_lo, 4), round(t_hi, 4)],
                    "count_only_ms": round(t_count, 4), "pairs_per_s": round(pairs / (t / 1e3), 1), "pairwise_ms": round(t_pair, 4),
                    "pairwise_min_max_ms": [round(p_lo, 4), round(p_hi, 4)], "mask_pairs": mp, "mask_fraction": round(mp / pairs, 4)}
            if conditioned:
                line["condition"] = "qgram_join_ms <= pairwise_ms"
                line["condition_met"] = bool(t <= t_pair)
                mid = S.MEASURE_ID["sorensen_dice"]
                mcount, mwhole, mnnz = prepared_match_join(ctx, mid, q, c, cutoff)
                (t2, _, _), (tm, m_lo, m_hi) = alternated(ctx, [whole, mwhole])
                line.update({"beside_match_join_ms": round(tm, 4), "match_join_min_max_ms": [round(m_lo, 4), round(m_hi, 4)], "match_join_nnz": mnnz,
                             "match_join_mask_pairs": match_mask_pairs("sorensen_dice", q, c, cutoff), "qgram_join_beside_ms": round(t2, 4)})
            emit(f, line)
        del pa, pb, pout
        if nself:
            x = host_column([s[:32] for s in near_duplicates(11, cands, nself)])
            mode = qgram_args("sorensen_dice", 2, True)
            count, whole, nnz = prepared_join(ctx, mode, x, x, 0.8, 1)
            (t, t_lo, t_hi), (t_count, _, _) = alternated(ctx, [whole, count])
            emit(f, {"bench": "qgram_join_self_upper", "kind": "sorensen_dice", "q": 2, "multiset": True, "rows": nself, "min_score": 0.8, "nnz": nnz,
                     "qgram_join_ms": round(t, 4), "qgram_join_min_max_ms": [round(t_lo, 4), round(t_hi, 4)], "count_only_ms": round(t_count, 4),
                     "pairs_per_s": round(nself * nself / (t / 1e3), 1)})
    ctx.close()


if __name__ == "__main__":
    main()
