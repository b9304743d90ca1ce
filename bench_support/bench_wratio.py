#!/usr/bin/env python3
"""wratio (measure 26) throughput, device-resident, one JSON line.

Every call is timed with hipEvents recorded on the context's stream around it (median of 10 timed repetitions behind 3 warm-ups).
The yardstick is the unrouted composition in the same process over the same rows: the sum of the six public calls a caller would
make without the routing -- indel, token_sort_ratio, token_set_ratio, partial_ratio, partial_token_sort_ratio and
partial_token_set_ratio -- each over the whole frame.  The condition of DESIGN.md section 18 is wratio < that sum.  Every host wait
of a call is inside its time.

Frame: 10 M rows.  Half are near: 1-4 tokens of 1-6 letters over abcdefgh (the generator of section 16's frame (a)), the second
column a shuffled copy with 40 % of its tokens edited, a 200 000-row block tiled on the device.  Half are far: section 15's frame
(b), a needle U{4..16} against a haystack U{32..128} of lowercase ASCII, planted with 0-2 substitutions in half of the rows.  The
line goes to stdout and to profiles/wratio_bench_lines.jsonl (replaced by a run at the full size).

    python bench_support/bench_wratio.py [--rows N] [--wratio-only]
(--wratio-only: one warm-up and three repetitions of the wratio call alone, for a kernel trace of its own)
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
from bench_support.bench_partial import needle_frame
from bench_support.bench_token import column, timed

DEV = torch.device("cuda", 0)
OUT = os.path.join(ROOT, "profiles", "wratio_bench_lines.jsonl")
BLOCK = 200_000
UNROUTED = ("indel", "token_sort_ratio", "token_set_ratio", "partial_ratio", "partial_token_sort_ratio", "partial_token_set_ratio")


def near_block(n, seed=2026):
    """section 16's token generator; b is always the shuffled, lightly edited copy of a"""
    rng = np.random.default_rng(seed)
    letters = "abcdefgh"

    def tok():
        return "".join(letters[int(k)] for k in rng.integers(0, 8, int(rng.integers(1, 7))))

    def edit(t):
        i, op, c = int(rng.integers(0, len(t))), int(rng.integers(0, 3)), letters[int(rng.integers(0, 8))]
        return (t[:i] + c + t[i + 1:], t[:i] + c + t[i:], (t[:i] + t[i + 1:]) or c)[op]

    A, B = [], []
    for _ in range(n):
        ta = [tok() for _ in range(int(rng.integers(1, 5)))]
        tb = [edit(t) if rng.random() < 0.4 else t for t in ta]
        rng.shuffle(tb)
        A.append(" ".join(ta))
        B.append(" ".join(tb))
    return A, B


def joined(x, y):
    """Two device columns (offsets int32, values uint8 + 64 bytes of padding, bytes) one behind the other."""
    off = torch.cat([x[0].to(torch.int64), y[0][1:].to(torch.int64) + x[2]]).to(torch.int32).contiguous()
    return off, torch.cat([x[1][:x[2]], y[1]]).contiguous(), x[2] + y[2]


def main():
    args = sys.argv[1:]
    rows = 10_000_000
    if "--rows" in args:
        i = args.index("--rows")
        rows = int(args[i + 1])
        del args[i:i + 2]
    only = "--wratio-only" in args
    half = rows // 2
    tiles = max(half // BLOCK, 1)
    A, B = near_block(BLOCK)
    na, nb = column(A, tiles), column(B, tiles)
    fa, fb = needle_frame(half)
    a = joined(na, (fa[0], fa[1], int(fa[0][-1])))
    b = joined(nb, (fb[0], fb[1], int(fb[0][-1])))
    n = tiles * BLOCK + half
    del na, nb, fa, fb
    torch.cuda.empty_cache()
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    with S.Context(0) as ctx:
        call = lambda m: (lambda: ctx.pairs_device(m, a[0], a[1], b[0], b[1], out))  # noqa: E731
        if only:
            ms = timed(ctx, call("wratio"), warmup=1, reps=3)
            print(json.dumps({"bench": "wratio", "rows": n, "wratio_ms": round(ms, 4), "routed": ctx.last_wratio_rows()}), flush=True)
            return
        res = {m: timed(ctx, call(m)) for m in UNROUTED}
        res["wratio"] = timed(ctx, call("wratio"))
        near, far = ctx.last_wratio_rows()
        total = sum(res[m] for m in UNROUTED)
        line = {"bench": "wratio", "desc": "%d M rows: half edited token copies (near), half needle U{4..16} in haystack U{32..128} (far)"
                % (n // 1_000_000), "rows": n, "bytes": a[2] + b[2], "near_rows": near, "far_rows": far}
        for k, v in res.items():
            line[k + "_ms"] = round(v, 4)
        line.update({"unrouted_sum_ms": round(total, 4), "wratio_over_unrouted_sum": round(res["wratio"] / total, 3),
                     "condition_routed_below_unrouted_sum": bool(res["wratio"] < total), "wratio_mpairs_s": round(n / res["wratio"] / 1e3, 1),
                     "device": torch.cuda.get_device_name(0)})
        print(json.dumps(line), flush=True)
        if rows == 10_000_000:
            with open(OUT, "w") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
