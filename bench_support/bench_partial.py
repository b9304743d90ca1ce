#!/usr/bin/env python3
"""Partial ratio (measure 10) throughput, device-resident, one JSON line per frame.

Every call is timed with hipEvents recorded on the context's stream around it (median of the timed repetitions).  A partial-ratio
call, like an Indel call, waits once for the stream after its first kernel (include/strsim_amd.h), so its time includes that host
round trip.

Frames:
  a   100 M rows U{1..32} lowercase ASCII (cfg2's generator): partial_ratio, indel on the same columns, and the alignment call.
  x   the baseline a caller has without this measure: the first 4 M pairs of frame (a) exploded into one row per window
      (needle, window; both directions for equal lengths), built on the device with torch, and `indel` through strsim_pairs_device
      on them -- against partial_ratio on the same 4 M pairs.  Building the exploded columns is not timed.  The maximum of the
      exploded scores per pair is compared with the fused score bit for bit.
  b   10 M rows, needle U{4..16}, haystack U{32..128} lowercase ASCII, the needle planted with 0-2 substitutions in half of the rows.
  c   1 M rows of mixed non-ASCII strings of up to 80 bytes (the wave tier), beside indel.
  d   frame (a)'s first column against the literal "jonathan", beside indel with the same literal.
Lines go to stdout and to profiles/partial_bench_lines.jsonl (replaced when every frame is run).

    python bench_support/bench_partial.py [--reps N] [frame ...]      (frames: a x b c d; default all)
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
OUT = os.path.join(ROOT, "profiles", "partial_bench_lines.jsonl")
EXPLODE_PAIRS = 4_000_000
EXPLODE_CHUNK = 500_000


def host_column(strings):
    o, v = S.pack_strings(strings)
    return (torch.from_numpy(o.view(np.int32)).to(DEV), torch.from_numpy(np.concatenate([v, np.zeros(64, np.uint8)])).to(DEV))


def timed(ctx, call, warmup, reps):
    """call() enqueues on the context's stream -> (median ms, last_wave_rows)."""
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
    return float(np.median(ms)), ctx.last_wave_rows


def time_pairs(ctx, measure, a, b, n, warmup, reps):
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    ms, wave_rows = timed(ctx, lambda: ctx.pairs_device(measure, a[0], a[1], b[0], b[1], out), warmup, reps)
    return ms, wave_rows, out


def time_alignment(ctx, a, b, n, warmup, reps):
    score = torch.empty(n, dtype=torch.float64, device=DEV)
    span = torch.empty((n, 4), dtype=torch.int32, device=DEV)
    ms, _ = timed(ctx, lambda: ctx.partial_alignment_device(a[0], a[1], b[0], b[1], score, span), warmup, reps)
    return ms, score


def cfg2_columns(n):
    _, _, law, lo, hi, seed = W.CONFIGS["cfg2"]
    oa, va, ob, vb, _, _ = W.device_columns(seed, law, lo, hi, 0, n, DEV)
    return (oa, va), (ob, vb)


def head(col, rows):
    """The first `rows` rows of a device column (offsets stay based at 0)."""
    off = col[0][:rows + 1].contiguous()
    return off, col[1]


def explode(a, b, rows):
    """One row per window of every pair: -> (needle column, window column, pair index of every exploded row)."""
    need_off, need_val, win_off, win_val, pair = [torch.zeros(1, dtype=torch.int64, device=DEV)], [], [torch.zeros(1, dtype=torch.int64, device=DEV)], [], []
    nbase = wbase = 0
    bshift = int(a[0][rows])
    vals = torch.cat([a[1][:bshift], b[1][:int(b[0][rows])]])
    for r0 in range(0, rows, EXPLODE_CHUNK):
        r1 = min(rows, r0 + EXPLODE_CHUNK)
        oa = a[0][r0:r1 + 1].to(torch.int64)
        ob = b[0][r0:r1 + 1].to(torch.int64)
        la, lb = oa[1:] - oa[:-1], ob[1:] - ob[:-1]
        # direction 0: the shorter string is the needle (a when equal); direction 1, equal lengths only: b is the needle
        a_needle = la <= lb
        eq = torch.nonzero(la == lb).flatten()
        m = torch.cat([torch.minimum(la, lb), la[eq]])
        n = torch.cat([torch.maximum(la, lb), la[eq]])
        nstart = torch.cat([torch.where(a_needle, oa[:-1], ob[:-1] + bshift), ob[:-1][eq] + bshift])
        hstart = torch.cat([torch.where(a_needle, ob[:-1] + bshift, oa[:-1]), oa[:-1][eq]])
        pid = torch.cat([torch.arange(r0, r1, device=DEV), eq + r0])
        cnt = torch.where(m > 0, n + m - 1, torch.zeros_like(m))  # (an empty string has no window: the pair scores 0.0, or 1.0 when both are)
        k = torch.arange(int(cnt.sum()), device=DEV) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
        mm, nn = torch.repeat_interleave(m, cnt), torch.repeat_interleave(n, cnt)
        i = torch.clamp(k - (mm - 1), min=0)
        wl = torch.minimum(k + 1, nn) - i

        def ragged(start, length):
            offs = torch.cumsum(length, 0)
            idx = torch.arange(int(offs[-1]), device=DEV) + torch.repeat_interleave(start - (offs - length), length)
            return offs, vals[idx]
        o, v = ragged(torch.repeat_interleave(nstart, cnt), mm)
        need_off.append(o + nbase); need_val.append(v); nbase += int(o[-1])
        o, v = ragged(torch.repeat_interleave(hstart, cnt) + i, wl)
        win_off.append(o + wbase); win_val.append(v); wbase += int(o[-1])
        pair.append(torch.repeat_interleave(pid, cnt))
        del k, mm, nn, i, wl, o, v
    pad = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert nbase < 2 ** 32 and wbase < 2 ** 32  # (uint32 offsets, carried as their bits in an int32 tensor)

    def u32_bits(x):
        return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)
    needle = (u32_bits(torch.cat(need_off)), torch.cat(need_val + [pad]))
    window = (u32_bits(torch.cat(win_off)), torch.cat(win_val + [pad]))
    return needle, window, torch.cat(pair)


def needle_frame(rows, seed=77):
    """Frame (b): needle U{4..16}, haystack U{32..128} lowercase ASCII; in half of the rows the needle is planted with 0-2
    substitutions."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g, device=DEV)  # noqa: E731
    nl, hl = ri(4, 17, (rows,)), ri(32, 129, (rows,))
    N = ri(97, 123, (rows, 16)).to(torch.uint8)
    H = ri(97, 123, (rows, 128)).to(torch.uint8)
    planted = ri(0, 2, (rows,)) == 1
    pos = (torch.rand(rows, generator=g, device=DEV) * (hl - nl + 1)).to(torch.int64)
    j = torch.arange(16, device=DEV)[None, :]
    copy = planted[:, None] & (j < nl[:, None])
    cols = pos[:, None] + j
    r = torch.arange(rows, device=DEV)[:, None].expand(-1, 16)
    H[r[copy], cols[copy]] = N[copy]
    for e in (1, 2):  # 0, 1 or 2 substitutions inside the planted copy
        sub = planted & (ri(0, 3, (rows,)) >= e)
        q = pos + (torch.rand(rows, generator=g, device=DEV) * nl).to(torch.int64)
        H[torch.nonzero(sub).flatten(), q[sub]] = ri(97, 123, (int(sub.sum()),)).to(torch.uint8)
    pad = torch.zeros(64, dtype=torch.uint8, device=DEV)

    def pack(M, length):
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(length, 0)]).to(torch.int32)
        return off, torch.cat([M[torch.arange(M.shape[1], device=DEV)[None, :] < length[:, None]], pad])
    return pack(N, nl), pack(H, hl)


def rate(n, ms):
    return round(n / ms / 1e3, 1)


def run_frame(ctx, f, reps):
    dev_name = torch.cuda.get_device_name(0)
    if f in ("a", "d", "x"):
        rows = 100_000_000
        a, b = cfg2_columns(rows)
        if f == "a":
            p_ms, wave_rows, p_out = time_pairs(ctx, "partial_ratio", a, b, rows, 3, reps)
            i_ms, _, _ = time_pairs(ctx, "indel", a, b, rows, 3, reps)
            al_ms, al_score = time_alignment(ctx, a, b, rows, 3, reps)
            same = bool(torch.equal(p_out.view(torch.int64), al_score.view(torch.int64)))
            return {"bench": "partial", "frame": "a", "desc": "100M U{1..32} ASCII (cfg2)", "rows": rows, "partial_ms": round(p_ms, 4),
                    "partial_mpairs_s": rate(rows, p_ms), "partial_wave_rows": int(wave_rows), "indel_ms": round(i_ms, 4),
                    "indel_mpairs_s": rate(rows, i_ms), "partial_over_indel_time": round(p_ms / i_ms, 3),
                    "alignment_ms": round(al_ms, 4), "alignment_over_partial_time": round(al_ms / p_ms, 3),
                    "alignment_score_equals_pairwise": same, "device": dev_name}
        if f == "d":
            lit = host_column(["jonathan"])
            p_ms, wave_rows, _ = time_pairs(ctx, "partial_ratio", a, lit, rows, 3, reps)
            i_ms, _, _ = time_pairs(ctx, "indel", a, lit, rows, 3, reps)
            return {"bench": "partial", "frame": "d", "desc": "100M U{1..32} ASCII x literal 'jonathan'", "rows": rows,
                    "partial_ms": round(p_ms, 4), "partial_mpairs_s": rate(rows, p_ms), "partial_wave_rows": int(wave_rows),
                    "indel_ms": round(i_ms, 4), "indel_mpairs_s": rate(rows, i_ms), "partial_over_indel_time": round(p_ms / i_ms, 3),
                    "device": dev_name}
        pairs = EXPLODE_PAIRS
        a4, b4 = head(a, pairs), head(b, pairs)
        needle, window, pair = explode(a4, b4, pairs)
        xrows = int(pair.numel())
        del a, b
        torch.cuda.empty_cache()
        x_ms, x_wave, x_out = time_pairs(ctx, "indel", needle, window, xrows, 3, reps)
        p_ms, _, p_out = time_pairs(ctx, "partial_ratio", a4, b4, pairs, 3, reps)
        best = torch.full((pairs,), -1.0, dtype=torch.float64, device=DEV).scatter_reduce(0, pair, x_out, "amax")
        la, lb = (a4[0][1:] - a4[0][:-1]), (b4[0][1:] - b4[0][:-1])
        best = torch.where((la == 0) | (lb == 0), ((la == 0) & (lb == 0)).to(torch.float64), best)
        differ = int((best.view(torch.int64) != p_out.view(torch.int64)).sum())
        return {"bench": "partial", "frame": "x", "desc": "first 4M pairs of frame (a): indel on the exploded windows vs partial_ratio",
                "pairs": pairs, "exploded_rows": xrows, "exploded_rows_per_pair": round(xrows / pairs, 2),
                "exploded_indel_ms": round(x_ms, 4), "exploded_wave_rows": int(x_wave), "partial_ms": round(p_ms, 4),
                "partial_over_exploded_time": round(p_ms / x_ms, 3), "condition_fused_at_most_half": bool(p_ms <= 0.5 * x_ms),
                "rows_where_max_of_exploded_differs": differ, "device": dev_name}
    if f == "b":
        rows = 10_000_000
        a, b = needle_frame(rows)
        p_ms, wave_rows, _ = time_pairs(ctx, "partial_ratio", a, b, rows, 2, reps)
        i_ms, _, _ = time_pairs(ctx, "indel", a, b, rows, 2, reps)
        return {"bench": "partial", "frame": "b", "desc": "10M needle U{4..16} in haystack U{32..128} ASCII, planted in half", "rows": rows,
                "partial_ms": round(p_ms, 4), "partial_mpairs_s": rate(rows, p_ms), "partial_wave_rows": int(wave_rows),
                "indel_ms": round(i_ms, 4), "partial_over_indel_time": round(p_ms / i_ms, 3), "device": dev_name}
    rows = 1_000_000
    A, B = gen.pairs(31, rows, gen.MIXED, 0, 80, max_bytes=80)
    a, b = host_column(A), host_column(B)
    p_ms, wave_rows, _ = time_pairs(ctx, "partial_ratio", a, b, rows, 3, reps)
    i_ms, i_wave, _ = time_pairs(ctx, "indel", a, b, rows, 3, reps)
    return {"bench": "partial", "frame": "c", "desc": "1M mixed non-ASCII <= 80 bytes", "rows": rows, "partial_ms": round(p_ms, 4),
            "partial_mpairs_s": rate(rows, p_ms), "partial_wave_rows": int(wave_rows), "indel_ms": round(i_ms, 4),
            "indel_wave_rows": int(i_wave), "partial_over_indel_time": round(p_ms / i_ms, 3), "device": dev_name}


def main():
    args = sys.argv[1:]
    reps = 10
    if args[:1] == ["--reps"]:
        reps = int(args[1])
        args = args[2:]
    frames = args or ["a", "x", "b", "c", "d"]
    lines = []
    with S.Context(0) as ctx:
        for f in frames:
            line = run_frame(ctx, f, reps)
            print(json.dumps(line), flush=True)
            lines.append(line)
            torch.cuda.empty_cache()
    if sorted(frames) == ["a", "b", "c", "d", "x"]:
        with open(OUT, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
