"""Child process of tests/test_osa_plugin_gpu.py: engine threads making small osa calls (and levenshtein ones in between) through the
plugin ABI with the combiner on (POLARS_STRSIM_COALESCE* from the parent's environment).  Every result is compared with
tests/osa_ref.py or the oracle bit for bit.  Prints one JSON line with the combiner's counters.

  osa_coalesce_child.py <threads> <calls per thread>"""
import ctypes as C
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "polars-strsim_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import numpy as np
import pyarrow as pa

import gen
import oracle_lib as O
import osa_ref as R
import strsim_amd
from strsim_amd import arrow_host as H

threads, calls = int(sys.argv[1]), int(sys.argv[2])
rng = np.random.default_rng(13)
frames = []
for k in range(12):
    n = int(rng.integers(1, 1500))
    A, B = gen.pairs(9000 + k, n, gen.ASCII_LOWER, 0, 32)
    if k % 3 == 0:
        A2, B2 = gen.pairs(9100 + k, max(1, n // 20), gen.MIXED, 0, 80)
        A, B = A + A2, B + B2
    An = [None if (k % 4 == 1 and i % 17 == 3) else a for i, a in enumerate(A)]
    fa, fb = pa.array(An, pa.string_view()), pa.array(B, pa.string_view())
    A0 = ["" if x is None else x for x in An]
    exp = {"osa": R.batch_numpy(A0, B), "levenshtein": O.batch_strings("levenshtein", A0, B, 2)}
    valid = np.array([x is not None for x in An])
    frames.append((fa, fb, exp, valid))

H.call_plugin("osa", frames[0][0], frames[0][1])
bad = []


def work(t):
    r = np.random.default_rng(200 + t)
    for c in range(calls):
        fa, fb, exp, valid = frames[int(r.integers(0, len(frames)))]
        m = "osa" if c % 3 else "levenshtein"
        g = H.call_plugin(m, fa, fb, parallel=True).combine_chunks()
        vals = np.asarray(g.to_numpy(zero_copy_only=False), dtype=np.float64)
        nulls = np.array(g.is_null().to_pylist())
        if len(g) != len(valid) or (nulls != ~valid).any() or (valid & (vals.view(np.uint64) != exp[m].view(np.uint64))).any():
            bad.append((t, c, m, len(g)))
            return


ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
for t in ts:
    t.start()
for t in ts:
    t.join()
out = (C.c_uint64 * 4)()
strsim_amd.lib()._polars_plugin_strsim_coalesce_stats(out)
print(json.dumps({"bad": bad, "combined_launches": int(out[0]), "calls_combined": int(out[1])}))
