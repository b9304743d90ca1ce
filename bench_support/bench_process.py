#!/usr/bin/env python3
"""default_process and processed scoring throughput, device-resident, one JSON line per frame.

Every call is timed with hipEvents recorded on the context's stream around it (median of 10 timed repetitions behind 3 warm-ups);
the one wait a transform makes for the stream (include/strsim_amd.h) is inside its time.  Two comparisons, in the same process and
on the same columns:
  (a) default_process of both columns against the token_sort transform of both columns: the same measure / scan / write structure,
      and default_process sorts nothing -- it must not be slower;
  (b) pairs_processed("indel") against the sum of the two transforms and "indel" over their output -- it must not be slower.
transform_hbm_share is (bytes read + bytes written, values and offsets, each pass counted) / time over the 8 TB/s peak.

Frames: (ascii) 10 M rows of mixed-case ASCII names of at most 32 bytes with punctuation, a 200 000-row block tiled on the device;
(mixed) the same frame with a tenth of the rows non-ASCII (Latin-1, Cyrillic and the two code points that grow).  Lines go to stdout
and to profiles/process_bench_lines.jsonl (replaced when every frame is run at the default size).

    python bench_support/bench_process.py [frame ...] [--rows N]      (frames: ascii mixed; default both)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import strsim_amd as S

DEV = torch.device("cuda", 0)
OUT = os.path.join(ROOT, "profiles", "process_bench_lines.jsonl")
BLOCK = 200_000
HBM_PEAK = 8.0e12  # bytes / s


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


WORDS = ["Apple", "Inc.", "GmbH", "Smith", "O'Neil", "AT&T", "Ltd", "van", "der", "Berg", "Co.", "LLC", "J.", "R.", "Mary-Ann", "St.",
         "and", "Sons", "Holdings", "PLC", "de", "la", "Cruz", "3M", "A1", "B2B"]
FOREIGN = ["École", "Zürich", "Жуков", "Łódź", "São", "Ⱥlpha", "Ⱦau", "Müller", "Ñandú"]


def names(n, foreign_share, seed):
    """(A, B): names of at most 32 bytes; B is A in another case with other punctuation, or another name."""
    rng = np.random.default_rng(seed)
    seps = [" ", ", ", " & ", "-", ". ", "  "]

    def name(words, s=""):
        for _ in range(int(rng.integers(1, 5))):
            w = words[int(rng.integers(0, len(words)))]
            t = s + (seps[int(rng.integers(0, len(seps)))] if s else "") + w
            if len(t.encode("utf-8")) > 32:
                break
            s = t
        return s

    A, B = [], []
    for _ in range(n):
        foreign = rng.random() < foreign_share
        words = WORDS + FOREIGN if foreign else WORDS
        lead = FOREIGN[int(rng.integers(0, len(FOREIGN)))] if foreign else ""   # (a foreign row holds a non-ASCII word at least)
        a = name(words, lead)
        b = (a.upper() if rng.random() < 0.5 else a.lower()).replace(", ", " ").replace(".", "") if rng.random() < 0.5 else name(words, lead)
        if len(b.encode("utf-8")) > 32:
            b = a
        A.append(a)
        B.append(b)
    return A, B


def frame(name, rows):
    share = 0.0 if name == "ascii" else 0.1
    A, B = names(BLOCK, share, 2024)
    tiles = max(rows // BLOCK, 1)
    non_ascii = sum(not s.isascii() for s in A) / len(A)
    desc = "%d M rows of mixed-case names of at most 32 bytes with punctuation, %.0f %% of the rows non-ASCII (tiled block of %d)" % (
        tiles * BLOCK // 1_000_000, 100 * non_ascii, BLOCK)
    return desc, column(A, tiles), column(B, tiles), tiles * BLOCK


def main():
    args = sys.argv[1:]
    rows = 10_000_000
    if "--rows" in args:
        i = args.index("--rows")
        rows = int(args[i + 1])
        del args[i:i + 2]
    frames = args or ["ascii", "mixed"]
    lines = []
    with S.Context(0) as ctx:
        for f in frames:
            desc, a, b, n = frame(f, rows)
            out = torch.empty(n, dtype=torch.float64, device=DEV)
            cap = lambda c: torch.empty(c[2] + c[2] // 2 + 64, dtype=torch.uint8, device=DEV)  # noqa: E731
            oa, va, ob, vb = torch.empty_like(a[0]), cap(a), torch.empty_like(b[0]), cap(b)
            ta, tva, tb, tvb = torch.empty_like(a[0]), torch.empty_like(a[1]), torch.empty_like(b[0]), torch.empty_like(b[1])

            def process():
                ctx.default_process_device(a[0], a[1], oa, va)
                ctx.default_process_device(b[0], b[1], ob, vb)

            def token_sort():
                ctx.token_sort_device(a[0], a[1], ta, tva)
                ctx.token_sort_device(b[0], b[1], tb, tvb)

            res = {"default_process_both_columns": timed(ctx, process)}
            wave_rows = 0
            for c, o, v in ((a, oa, va), (b, ob, vb)):
                ctx.default_process_device(c[0], c[1], o, v)
                wave_rows += ctx.last_process_wave_rows
            ctx.synchronize()
            out_bytes = int(oa[-1]) + int(ob[-1])
            res["token_sort_both_columns"] = timed(ctx, token_sort)
            res["indel_over_processed"] = timed(ctx, lambda: ctx.pairs_device("indel", oa, va, ob, vb, out))
            res["pairs_processed_indel"] = timed(ctx, lambda: ctx.pairs_processed_device("indel", a[0], a[1], b[0], b[1], out))
            res["indel_raw"] = timed(ctx, lambda: ctx.pairs_device("indel", a[0], a[1], b[0], b[1], out))
            # the transform's traffic: the measuring pass reads the offsets and the values and writes the lengths, the scan reads and
            # writes them (twice read), the writing pass reads the old and the new offsets and the values and writes the new values
            traffic = 2 * (a[2] + b[2]) + out_bytes + 4 * 2 * n * (1 + 1 + 3 + 2)
            line = {"bench": "process", "frame": f, "desc": desc, "rows": n, "bytes": a[2] + b[2], "processed_bytes": out_bytes}
            for k, v in res.items():
                line[k + "_ms"] = round(v, 4)
            two_step = res["default_process_both_columns"] + res["indel_over_processed"]
            line.update({"process_over_token_sort": round(res["default_process_both_columns"] / res["token_sort_both_columns"], 3),
                         "not_slower_than_token_sort": bool(res["default_process_both_columns"] <= res["token_sort_both_columns"]),
                         "pairs_processed_over_two_step": round(res["pairs_processed_indel"] / two_step, 3),
                         "not_slower_than_two_step": bool(res["pairs_processed_indel"] <= two_step),
                         "transform_mrows_s": round(2 * n / res["default_process_both_columns"] / 1e3, 1),
                         "transform_traffic_bytes": int(traffic),
                         "transform_hbm_share": round(traffic / (res["default_process_both_columns"] * 1e-3) / HBM_PEAK, 4),
                         "process_wave_rows": int(wave_rows), "device": torch.cuda.get_device_name(0)})
            print(json.dumps(line), flush=True)
            lines.append(line)
            del a, b, out, oa, va, ob, vb, ta, tva, tb, tvb
            torch.cuda.empty_cache()
    if sorted(frames) == ["ascii", "mixed"] and rows == 10_000_000:
        with open(OUT, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
