#!/usr/bin/env python3
"""token_sort_ratio / token_set_ratio (measures 14 and 16) throughput, device-resident, one JSON line per frame.

Every call is timed with hipEvents recorded on the context's stream around it (median of 10 timed repetitions behind 3 warm-ups).
The yardstick is "indel" in the same process over the PRE-NORMALISED columns of the same rows (token_sort_device applied once,
outside the timed region): those kernels are untouched by the token measures, so token_sort_ratio / indel_prenormalised is what the
transform costs on top of the alignment.  The aim of DESIGN.md section 16 is at most 2.0.  A token call waits for the stream twice
(include/strsim_amd.h); both round trips are inside its time.

Frames: (a) 100 M rows of the generator of tests/token_ref.py (1-4 tokens of 1-6 letters over abcdefgh, the second column a shuffled,
lightly edited copy in half of the rows), a 200 000-row block tiled on the device; (lit) frame (a)'s first column against a
literal; (mixed) 1 M rows of 1-4 tokens over a Latin / Cyrillic / CJK alphabet with multi-byte whitespace, which the
one-string-per-wave tier takes.  Lines go to stdout and to profiles/token_bench_lines.jsonl (replaced when every frame is run).

    python bench_support/bench_token.py [frame ...] [--rows N]      (frames: a lit mixed; default all)
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
import token_ref as R

DEV = torch.device("cuda", 0)
OUT = os.path.join(ROOT, "profiles", "token_bench_lines.jsonl")
BLOCK = 200_000


def column(strings, tiles=1):
    """A device column of `strings` repeated `tiles` times -> (offsets int32, values uint8, bytes)."""
    off, val = S.pack_strings(strings)
    total = int(off[-1])
    o = torch.from_numpy(off.astype(np.int64)).to(DEV)
    offs = (o[:-1].unsqueeze(0) + torch.arange(tiles, device=DEV, dtype=torch.int64).unsqueeze(1) * total).reshape(-1)
    offs = torch.cat([offs, torch.tensor([tiles * total], device=DEV, dtype=torch.int64)]).to(torch.int32).contiguous()
    vals = torch.from_numpy(val).to(DEV).repeat(tiles)
    return offs, torch.cat([vals, torch.zeros(64, dtype=torch.uint8, device=DEV)]).contiguous(), tiles * total


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


def mixed_frame(n, seed=7):
    rng = np.random.default_rng(seed)
    letters = list("abcdefgh") + list("жукб") + list("漢字東")
    seps = [" ", " ", "\u00a0", "\u3000", "\u2003", "\t"]

    def tok():
        return "".join(letters[int(k)] for k in rng.integers(0, len(letters), int(rng.integers(1, 7))))

    A, B = [], []
    for _ in range(n):
        ta = [tok() for _ in range(int(rng.integers(1, 5)))]
        tb = list(ta) if rng.random() < 0.5 else [tok() for _ in range(int(rng.integers(1, 5)))]
        rng.shuffle(tb)
        A.append(seps[int(rng.integers(0, len(seps)))].join(ta))
        B.append(seps[int(rng.integers(0, len(seps)))].join(tb))
    return A, B


def frame(name, rows):
    if name in ("a", "lit"):
        A, B = R.gen_frame(2024, BLOCK)
        tiles = max(rows // BLOCK, 1)
        a = column(A, tiles)
        if name == "a":
            return "%d M rows, 1-4 tokens of 1-6 letters over abcdefgh (tiled block of %d)" % (tiles * BLOCK // 1_000_000, BLOCK), a, column(B, tiles), tiles * BLOCK
        return "the first column of frame (a) x literal 'dcab ab fgh'", a, column(["dcab ab fgh"]), tiles * BLOCK
    n = min(rows, 1_000_000)
    A, B = mixed_frame(BLOCK)
    tiles = max(n // BLOCK, 1)
    return "%d M rows, 1-4 tokens over Latin / Cyrillic / CJK with multi-byte whitespace" % (tiles * BLOCK // 1_000_000), column(A, tiles), column(B, tiles), tiles * BLOCK


def main():
    args = sys.argv[1:]
    rows = 100_000_000
    if "--rows" in args:
        i = args.index("--rows")
        rows = int(args[i + 1])
        del args[i:i + 2]
    frames = args or ["a", "lit", "mixed"]
    lines = []
    with S.Context(0) as ctx:
        for f in frames:
            desc, a, b, n = frame(f, rows)
            out = torch.empty(n, dtype=torch.float64, device=DEV)
            na, nb = ctx.token_sort_device(a[0], a[1]), ctx.token_sort_device(b[0], b[1])
            ctx.synchronize()
            res = {"indel_prenormalised": timed(ctx, lambda: ctx.pairs_device("indel", na[0], na[1], nb[0], nb[1], out))}
            indel_wave = ctx.last_wave_rows
            res["indel_raw"] = timed(ctx, lambda: ctx.pairs_device("indel", a[0], a[1], b[0], b[1], out))
            res["token_sort_ratio"] = timed(ctx, lambda: ctx.pairs_device("token_sort_ratio", a[0], a[1], b[0], b[1], out))
            sort_wave = ctx.last_token_wave_rows
            res["token_set_ratio"] = timed(ctx, lambda: ctx.pairs_device("token_set_ratio", a[0], a[1], b[0], b[1], out))
            set_wave = ctx.last_token_wave_rows
            oa, va = torch.empty_like(a[0]), torch.empty_like(a[1])
            ob, vb = torch.empty_like(b[0]), torch.empty_like(b[1])

            def transform():
                ctx.token_sort_device(a[0], a[1], oa, va)
                ctx.token_sort_device(b[0], b[1], ob, vb)

            res["token_sort_both_columns"] = timed(ctx, transform)
            line = {"bench": "token", "frame": f, "desc": desc, "rows": n, "bytes": a[2] + b[2]}
            for k, v in res.items():
                line[k + "_ms"] = round(v, 4)
            line.update({"sort_over_indel_prenormalised": round(res["token_sort_ratio"] / res["indel_prenormalised"], 3),
                         "set_over_indel_prenormalised": round(res["token_set_ratio"] / res["indel_prenormalised"], 3),
                         "token_sort_ratio_mpairs_s": round(n / res["token_sort_ratio"] / 1e3, 1),
                         "token_set_ratio_mpairs_s": round(n / res["token_set_ratio"] / 1e3, 1),
                         "indel_wave_rows": int(indel_wave), "sort_token_wave_rows": int(sort_wave), "set_token_wave_rows": int(set_wave),
                         "device": torch.cuda.get_device_name(0)})
            print(json.dumps(line), flush=True)
            lines.append(line)
            del a, b, na, nb, out, oa, va, ob, vb
            torch.cuda.empty_cache()
    if sorted(frames) == ["a", "lit", "mixed"] and rows == 100_000_000:
        with open(OUT, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
