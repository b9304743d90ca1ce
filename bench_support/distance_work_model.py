#!/usr/bin/env python3
"""The work k_dist_wave does on frame (d) of bench_distance.py, counted on the CPU: the host build of dist_column
(tests/cpu_harness/distance_harness.cpp) runs a sample of pairs from the same generator and counts, per measure and max_distance,
the text columns run and the word steps taken, relative to no cutoff, split by near-duplicate and unrelated pairs.  DESIGN.md §12
compares these counts with the measured times.  No GPU needed.

    python bench_support/distance_work_model.py [pairs] [K,K,...]      (default 600 pairs; cutoffs unbounded,999,64,16,4)
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_support.bench_distance import long_pairs  # noqa: E402

U = 0xFFFFFFFF


def harness(tmp):
    so = os.path.join(tmp, "libdist_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "polars-strsim_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "cpu_harness", "distance_harness.cpp")])
    L = C.CDLL(so)
    L.dist_block_distance.restype = C.c_uint32
    L.dist_block_distance.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]
    return L


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    cutoffs = [U if c == "unbounded" else int(c) for c in (sys.argv[2] if len(sys.argv) > 2 else "unbounded,999,64,16,4").split(",")]
    A, B = long_pairs(n)
    X = [np.frombuffer(a, dtype=np.uint8).astype(np.uint32) for a in A]
    Y = [np.frombuffer(b, dtype=np.uint8).astype(np.uint32) for b in B]
    with tempfile.TemporaryDirectory() as tmp:
        L = harness(tmp)
        for tr, m in ((0, "levenshtein"), (1, "osa")):
            base = None
            for k in cutoffs:
                cnt = {"near": [0, 0, 0, 0], "unrelated": [0, 0, 0, 0]}  # columns, word steps, pairs run at all, pairs with d <= k
                for i, (x, y) in enumerate(zip(X, Y)):
                    cols, words = C.c_uint64(0), C.c_uint64(0)
                    d = L.dist_block_distance(x.ctypes.data, len(x), y.ctypes.data, len(y), tr, k, C.byref(cols), C.byref(words))
                    c = cnt["near" if i % 2 == 0 else "unrelated"]
                    c[0] += cols.value
                    c[1] += words.value
                    c[2] += cols.value > 0
                    c[3] += k == U or d <= k
                cols = cnt["near"][0] + cnt["unrelated"][0]
                words = cnt["near"][1] + cnt["unrelated"][1]
                if base is None:
                    base = (cols, words)
                print(json.dumps({"measure": m, "max_distance": "unbounded" if k == U else k, "pairs": n,
                                  "columns_vs_unbounded": round(cols / base[0], 3), "word_steps_vs_unbounded": round(words / base[1], 3),
                                  "words_per_column": round(words / max(cols, 1), 2),
                                  "near": {"columns": cnt["near"][0], "word_steps": cnt["near"][1], "pairs_run": cnt["near"][2],
                                           "pairs_within_k": cnt["near"][3]},
                                  "unrelated": {"columns": cnt["unrelated"][0], "word_steps": cnt["unrelated"][1],
                                                "pairs_run": cnt["unrelated"][2], "pairs_within_k": cnt["unrelated"][3]}}), flush=True)


if __name__ == "__main__":
    main()
