#!/usr/bin/env python3
"""Differential fuzz of the HIP path against the CPU oracle: random scripts x length classes x measures x literal sides.
Usage: python tests/fuzz_gpu.py [seconds] [seed] [family set].  Exits non-zero on the first mismatch (prints the row).
Family sets: "classic" (the default: the five classic measures against the oracle) and "extended" (osa, indel, partial_ratio with
its alignment, both token ratios, the token_sort transform, the three distances with a random max_distance and small searches,
against the *_ref models)."""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-strsim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the oracle is test infrastructure: this script lives in tests/
import numpy as np

import gen
import oracle_lib as O
import strsim_amd as S

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = random.Random(seed)
ALPHABETS = {
    "a-z": gen.ASCII_LOWER, "ab": "ab", "ascii": "".join(chr(c) for c in range(1, 128)),
    "latin1": gen.ASCII_LOWER + "éèüñß ", "cyrillic": "".join(chr(c) for c in range(0x430, 0x450)) + " ",
    "mixed": gen.MIXED, "cjk": "".join(chr(c) for c in range(0x4E00, 0x4E40)) + "ab",
    "astral": "abé" + "".join(chr(c) for c in range(0x1F600, 0x1F610)),
}
CLASSES = [(0, 8, 20000), (0, 40, 20000), (20, 140, 6000), (100, 1100, 600), (900, 2600, 60), (0, 1100, 1500)]
ctx = S.Context(0)


def bounds_violations():
    """Lab build only (EXTRA="-DSTRSIM_LAB -DSTRSIM_BOUNDS", selected with STRSIM_AMD_LIB): the kernels' address-check records, read and
    cleared -> [(unit, hits, kernel, site, row, value, lo, hi)] of the units that saw a violation.  The product library has no such
    symbols: []."""
    import ctypes as C
    out = []
    for unit in ("kernels", "codec"):
        f = getattr(S.lib(), "strsim_debug_bounds_" + unit, None)
        if f is None:
            continue
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        rec = (C.c_ulonglong * 6)()
        assert f(rec) == 0
        if rec[0]:
            out.append((unit, rec[0], rec[1] >> 32, rec[1] & 0xFFFFFFFF, rec[2], hex(rec[3]), hex(rec[4]), hex(rec[5])))
    return out


CHECKED = hasattr(S.lib(), "strsim_debug_bounds_kernels")
family_set = sys.argv[3] if len(sys.argv) > 3 else "classic"
if family_set not in ("classic", "extended"):
    sys.exit(f"unknown family set {family_set!r} (classic, extended)")

EXT_FAMILIES = ["osa", "indel", "partial_ratio", "token_sort_ratio", "token_set_ratio", "token_sort", "distance:levenshtein",
                "distance:osa", "distance:indel", "nearest", "extract", "best_match"]
# (lo, hi, rows): lengths on both sides of the lane caps of the newer measures -- 32 (partial_ratio, the searches), 64 (osa, the token
# measures, the Levenshtein / OSA distances), 128 (indel) -- and of the wave kernels' 1 024; rows so that the models' DPs take well
# under a second a round.  The partial ratio's model scores every window: fewer rows for it.
EXT_CLASSES = [(0, 8, 2000), (24, 40, 1200), (56, 72, 500), (120, 136, 200), (0, 140, 300), (1000, 1050, 10), (0, 1100, 20)]
EXT_CLASSES_PARTIAL = [(0, 8, 2000), (24, 40, 300), (56, 72, 60), (120, 136, 10), (0, 140, 40)]
EXT_CLASSES_SEARCH = [(0, 12, 48, 200), (0, 34, 32, 100), (28, 36, 24, 60)]  # (lo, hi, queries, candidates): 32 bytes inside


def extended():
    """One family a round against its model (tests/relation_checks.py: ModelBackend, the C forms of the *_ref models, so rows of a
    thousand characters are within reach)."""
    import relation_checks as RC
    model, gpu = RC.ModelBackend(), RC.GpuBackend(ctx)
    t_end, rounds = time.time() + budget, 0

    def fail(what, detail):
        print(f"MISMATCH round {rounds + 1}: {what} seed={seed}: {detail}")
        sys.exit(1)

    def rows_differ(what, got, exp, A2, B2, bits):
        got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
        ne = got.view(np.uint64) != exp.view(np.uint64) if bits else got != exp
        bad = np.nonzero(ne.reshape(len(ne), -1).any(axis=1))[0]
        if bad.size:
            i = int(bad[0])
            fail(what, f"{bad.size} rows; row {i}: a={A2[i]!r} b={B2[i]!r} got={got[i].tolist()!r} exp={exp[i].tolist()!r}")

    while time.time() < t_end:
        family = rng.choice(EXT_FAMILIES)
        name = rng.choice(list(ALPHABETS))
        alpha = ALPHABETS[name]
        if family.startswith("token") or family == "extract":  # (tokens need whitespace: one character in six)
            alpha = alpha + " " * max(1, len(alpha) // 5)
        p_edit = rng.choice([0.2, 0.5, 0.9])
        if family in ("nearest", "extract", "best_match"):
            lo, hi, nq, nc = rng.choice(EXT_CLASSES_SEARCH)
            Q, Q2 = gen.pairs(rng.randrange(1 << 30), rng.randrange(1, nq + 1), alpha, lo, hi, p_edit=p_edit, p_same=0.05)
            Cs = (Q2 + gen.pairs(rng.randrange(1 << 30), nc, alpha, lo, hi)[0])[:rng.randrange(1, nc + 1)]
            rng.shuffle(Cs)
            k = rng.choice([1, 3, 16])
            if family == "nearest":
                m, cut = rng.choice(["levenshtein", "osa"]), rng.choice([0, 1, 2, 5, None])
            elif family == "extract":
                m, cut = rng.choice(["indel", "token_sort_ratio"]), rng.choice([None, 0.3, 0.6, 0.9])
            else:
                m, cut = rng.choice(O.MEASURES), rng.choice([None, 0.3, 0.6, 0.9])
            what = f"{family} {m} {name} [{lo},{hi}] queries={len(Q)} candidates={len(Cs)} k={k} cutoff={cut}"
            if os.environ.get("STRSIM_FUZZ_VERBOSE"):
                print(f"round {rounds + 1}: {what}", flush=True)
            gi, gv = getattr(gpu, family)(m, Q, Cs, k, cut)
            ei, ev = getattr(model, family)(m, Q, Cs, k, cut)
            differ = (gi != ei) | ((ei >= 0) & (gv.view(np.uint64) != ev.view(np.uint64) if gv.dtype == np.float64 else gv != ev))
            bad = np.nonzero(differ.any(axis=1))[0]
            if bad.size:
                i = int(bad[0])
                fail(what, f"{bad.size} queries; query {i}: q={Q[i]!r} got={gi[i].tolist()} / {gv[i].tolist()} exp={ei[i].tolist()} / "
                           f"{ev[i].tolist()} candidates={[Cs[j] for j in set(gi[i].tolist() + ei[i].tolist()) if j >= 0]!r}")
        else:
            lo, hi, n = rng.choice(EXT_CLASSES_PARTIAL if family == "partial_ratio" else EXT_CLASSES)
            n = rng.randrange(1, n + 1)
            A, B = gen.pairs(rng.randrange(1 << 30), n, alpha, lo, hi, p_edit=p_edit, p_same=0.05)
            side = rng.choice(["none", "none", "left", "right"]) if family != "token_sort" else "none"
            if side == "left":
                A = [A[rng.randrange(n)]]
            elif side == "right":
                B = [B[rng.randrange(n)]]
            k = rng.choice([0, 1, 2, 5, None]) if family.startswith("distance:") else None
            what = f"{family} {name} [{lo},{hi}] n={n} literal={side}" + (f" max_distance={k}" if family.startswith("distance:") else "")
            if os.environ.get("STRSIM_FUZZ_VERBOSE"):
                print(f"round {rounds + 1}: {what}", flush=True)
            A2, B2 = RC.bcast(A, B)
            if family == "token_sort":
                got, exp = gpu.token_sort(A), model.token_sort(A)
                bad = [i for i in range(n) if got[i] != exp[i]]
                if bad:
                    fail(what, f"{len(bad)} rows; row {bad[0]}: a={A[bad[0]]!r} got={got[bad[0]]!r} exp={exp[bad[0]]!r}")
            elif family.startswith("distance:"):
                m = family.split(":")[1]
                rows_differ(what, gpu.dist(m, A, B, k), model.dist(m, A, B, k), A2, B2, False)
            else:
                rows_differ(what, gpu.sim(family, A, B), model.sim(family, A, B), A2, B2, True)
                if family == "partial_ratio":
                    (gs, gp), (es, ep) = gpu.partial(A, B), model.partial(A, B)
                    rows_differ(what + " alignment score", gs, es, A2, B2, True)
                    rows_differ(what + " alignment span", gp, ep, A2, B2, False)
        gpu.log.clear()
        viol = bounds_violations()
        if viol:
            print(f"ADDRESS OUT OF BOUNDS round {rounds + 1}: {what} seed={seed}: (unit, hits, kernel, site, row, value, lo, hi) = {viol}")
            sys.exit(2)
        rounds += 1
    print(f"fuzz ok: {rounds} rounds in {budget:.0f} s (seed {seed}, extended){', every address checked (lab build)' if CHECKED else ''}")


if family_set == "extended":
    extended()
    sys.exit(0)
t_end = time.time() + budget
rounds = 0
while time.time() < t_end:
    name = rng.choice(list(ALPHABETS))
    alpha = ALPHABETS[name]
    lo, hi, n = rng.choice(CLASSES)
    n = rng.randrange(1, n + 1)
    measure = rng.choice(O.MEASURES)
    A, B = gen.pairs(rng.randrange(1 << 30), n, alpha, lo, hi, p_edit=rng.choice([0.2, 0.5, 0.9]), p_same=0.05)
    side = rng.choice(["none", "none", "left", "right"])
    if side == "left":
        A = [A[rng.randrange(n)]]
    elif side == "right":
        B = [B[rng.randrange(n)]]
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    if os.environ.get("STRSIM_FUZZ_VERBOSE"):  # (a GPU fault kills the process: say what was running)
        print(f"round {rounds + 1}: {measure} {name} [{lo},{hi}] n={n} literal={side} bytes a={len(av)} b={len(bv)}", flush=True)
    got = ctx.pairs_host(measure, ao, av, bo, bv)
    viol = bounds_violations()
    if viol:
        print(f"ADDRESS OUT OF BOUNDS round {rounds + 1}: {measure} {name} [{lo},{hi}] n={n} literal={side} seed={seed}: "
              f"(unit, hits, kernel, site, row, value, lo, hi) = {viol}")
        sys.exit(2)
    A2 = A * n if len(A) == 1 else A
    B2 = B * n if len(B) == 1 else B
    exp = O.batch_strings(measure, A2, B2, 16)
    bad = np.nonzero(got.view(np.uint64) != exp.view(np.uint64))[0]
    rounds += 1
    if bad.size:
        i = int(bad[0])
        print(f"MISMATCH round {rounds}: {measure} {name} [{lo},{hi}] n={n} literal={side}: {bad.size} rows; row {i}: "
              f"a={A2[i]!r} b={B2[i]!r} got={got[i]!r} exp={exp[i]!r}")
        sys.exit(1)
print(f"fuzz ok: {rounds} rounds in {budget:.0f} s (seed {seed}){', every address checked (lab build)' if CHECKED else ''}")
