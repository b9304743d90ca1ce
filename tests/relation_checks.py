"""The relations of tests/relations.py stated once, over a backend: ModelBackend (the oracle and the *_ref models, for
tests/test_relations_cpu.py) or GpuBackend (strsim_amd.Context, for tests/test_relations_gpu.py).  Every comparison is exact: f64
results as their 64 bits, distances, spans and indices as integers.

A backend takes lists of str (one side may be a literal: a list of one string) and returns numpy arrays.  `role` ("base": the
untouched lane-class pairs, "image": transformed ones that left the lane tier, "edge": transformed ones that sit at its last length,
"mixed": some of each) is what GpuBackend files each call's tier counters under, so that the GPU
tests can assert that the image really left the base's tier; the models ignore it.
"""
import random

import numpy as np

import relations as T

CLASSIC = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")
NEWER = ("osa", "indel", "partial_ratio")
TOKEN = ("token_sort_ratio", "token_set_ratio")
SIMILARITIES = CLASSIC + NEWER + TOKEN
DISTANCES = ("levenshtein", "osa", "indel")
REVERSAL_SIMS = ("levenshtein", "osa", "indel", "jaccard", "sorensen_dice")
SWAP_SIMS = ("osa", "indel", "partial_ratio", "token_sort_ratio", "token_set_ratio")
# max_distance cases: the generator's edited copies lie within them, its independent pairs beyond (an Indel substitution costs 2)
CUTOFFS = {"levenshtein": (1, 2, 5), "osa": (1, 2, 5), "indel": (2, 4, 8)}
KS = {m: (0,) + CUTOFFS[m] + (None,) for m in DISTANCES}


def bcast(A, B):
    n = max(len(A), len(B))
    return (list(A) * n if len(A) == 1 and n != 1 else list(A)), (list(B) * n if len(B) == 1 and n != 1 else list(B))


def same_bits(got, exp, A, B, what):
    got, exp = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    if bad.size:
        A, B = bcast(A, B)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size}/{got.size} rows differ; row {i}: a={A[i]!r} b={B[i]!r}: {got[i]!r} != {exp[i]!r}")


def same_ints(got, exp, A, B, what):
    got, exp = np.asarray(got).astype(np.int64), np.asarray(exp).astype(np.int64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    if bad.size:
        A, B = bcast(A, B)
        i = int(bad[0][0])
        raise AssertionError(f"{what}: {len(bad)} entries differ; row {i}: a={A[i]!r} b={B[i]!r}: {got[i].tolist()} != {exp[i].tolist()}")


def same_lists(got, exp, what):
    """Two search results (index int64 [n, k] with -1 in empty slots, value [n, k]): the same slots filled, with the same candidates and
    the same values (scores by their bits)."""
    gi, gv = got
    ei, ev = exp
    assert gi.shape == ei.shape and gv.shape == ev.shape, what
    full = ei >= 0
    if gv.dtype == np.float64:
        differ = np.ascontiguousarray(gv).view(np.uint64) != np.ascontiguousarray(ev).view(np.uint64)
    else:
        differ = gv != ev
    bad = np.argwhere((gi != ei) | (full & differ))
    assert bad.size == 0, "%s: query %d differs: %s / %s != %s / %s" % (
        what, bad[0][0], gi[bad[0][0]].tolist(), gv[bad[0][0]].tolist(), ei[bad[0][0]].tolist(), ev[bad[0][0]].tolist())


def call(be, kind, m, A, B, k=None, role=None):
    return be.sim(m, A, B, role=role) if kind == "sim" else be.dist(m, A, B, k, role=role)


def same(kind, got, exp, A, B, what):
    (same_bits if kind == "sim" else same_ints)(got, exp, A, B, what)


def col(f, X, *args):
    return [f(s, *args) for s in X]


# ---- relabel ----

def relabel_sim(be, m, base, A, B):
    same_bits(be.sim(m, col(T.relabel, A, base), col(T.relabel, B, base), role="image"), be.sim(m, A, B, role="base"), A, B,
              f"{m} relabelled by {base:#x}")


def relabel_dist(be, m, base, A, B):
    A2, B2 = col(T.relabel, A, base), col(T.relabel, B, base)
    for k in KS[m]:
        same_ints(be.dist(m, A2, B2, k, role="image"), be.dist(m, A, B, k, role="base"), A, B, f"{m} distance k={k} relabelled by {base:#x}")


def relabel_partial(be, base, A, B):
    s0, p0 = be.partial(A, B, role="base")
    s1, p1 = be.partial(col(T.relabel, A, base), col(T.relabel, B, base), role="image")
    same_bits(s1, s0, A, B, f"partial alignment score relabelled by {base:#x}")
    same_ints(p1, p0, A, B, f"partial alignment span relabelled by {base:#x}")


def relabel_token_sort(be, base, X):
    got = col(T.unrelabel, be.token_sort(col(T.relabel, X, base), role="image"), base)
    assert got == be.token_sort(X, role="base"), f"token_sort relabelled by {base:#x}"


# ---- common affix, reversal, swap, order of the distances ----

def affix_dist(be, m, A, B, A2, B2, what, role="image"):
    """(A2, B2) are (A, B) with common affixes: the same distances at every cutoff, min(d, k + 1) included."""
    for k in KS[m]:
        same_ints(be.dist(m, A2, B2, k, role=role), be.dist(m, A, B, k, role="base"), A2, B2, f"{m} distance k={k} {what}")


def reversal(be, kind, m, A, B):
    A2, B2 = col(T.reverse, A), col(T.reverse, B)
    for k in (KS[m] if kind == "dist" else (None,)):
        same(kind, call(be, kind, m, A2, B2, k), call(be, kind, m, A, B, k), A, B, f"{m} {kind} k={k} reversed")


def swap(be, kind, m, A, B):
    for k in (KS[m] if kind == "dist" else (None,)):
        same(kind, call(be, kind, m, B, A, k), call(be, kind, m, A, B, k), A, B, f"{m} {kind} k={k} swapped")


def distance_order(be, A, B):
    """| |a| - |b| | <= osa <= lev <= indel <= 2 lev, lev <= max(|a|, |b|), indel = |a| + |b| (mod 2): three kernels agree."""
    la, lb = np.array([len(a) for a in A]), np.array([len(b) for b in B])
    lev, osa, ind = (be.dist(m, A, B, None).astype(np.int64) for m in DISTANCES)
    for name, ok in (("| |a| - |b| | <= osa", np.abs(la - lb) <= osa), ("osa <= lev", osa <= lev), ("lev <= indel", lev <= ind),
                     ("indel <= 2 lev", ind <= 2 * lev), ("lev <= max(|a|, |b|)", lev <= np.maximum(la, lb)),
                     ("indel = |a| + |b| (mod 2)", (ind - la - lb) % 2 == 0)):
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (name, A[bad[0]], B[bad[0]], int(lev[bad[0]]), int(osa[bad[0]]), int(ind[bad[0]]))
    return lev, osa, ind


# ---- partial ratio ----

def partial_spans_are_indel(be, A, B):
    """Both strings non-empty: indel(a[ss:se], b[ds:de]) by the pairwise call is the alignment's score."""
    score, span = be.partial(A, B)
    rows = [i for i in range(len(A)) if A[i] and B[i]]
    X = [A[i][int(span[i][0]):int(span[i][1])] for i in rows]
    Y = [B[i][int(span[i][2]):int(span[i][3])] for i in rows]
    same_bits(be.sim("indel", X, Y), score[rows], X, Y, "indel of the partial alignment's spans")
    same_bits(be.sim("partial_ratio", A, B), score, A, B, "partial_ratio against its alignment's score")
    return len(rows)


def partial_contained(be, needles, haystacks):
    """partial_ratio(a, x + a + y) is 1.0 for a non-empty a, on either side."""
    one = np.ones(len(needles))
    same_bits(be.sim("partial_ratio", needles, haystacks, role="mixed"), one, needles, haystacks, "partial_ratio of a contained needle")
    same_bits(be.sim("partial_ratio", haystacks, needles, role="mixed"), one, haystacks, needles, "partial_ratio of a contained needle, swapped")


def partial_at_least_indel(be, A, B):
    """|a| == |b|: the whole of b is one of the windows."""
    assert all(len(a) == len(b) for a, b in zip(A, B))
    p, s = be.sim("partial_ratio", A, B), be.sim("indel", A, B)
    bad = np.flatnonzero(p < s)
    assert bad.size == 0, (A[bad[0]], B[bad[0]], p[bad[0]], s[bad[0]])


# ---- token measures ----

def token_image(seed, X, whitespace, mode):
    """One column's tokens permuted and joined again: "shuffle" runs of 1..3 whitespace characters, "spread" one run of 65 more (the
    string has more than 64 characters), "copies" every token four times (a string of five tokens has 20)."""
    rng = random.Random(seed)
    if mode == "spread":
        return [T.spread_tokens(rng, s, whitespace, 65) for s in X]
    return [T.shuffle_tokens(rng, s, whitespace, copies=4 if mode == "copies" else 1) for s in X]


def token_invariance(be, m, A, B, A2, B2, what, role="image"):
    same_bits(be.sim(m, A2, B2, role=role), be.sim(m, A, B, role="base"), A2, B2, f"{m} {what}")


def token_sort_idempotent(be, X, role=None):
    once = be.token_sort(X, role=role)
    assert be.token_sort(once) == once
    return once


def token_sort_ratio_is_indel(be, A, B, role=None):
    same_bits(be.sim("token_sort_ratio", A, B, role=role), be.sim("indel", be.token_sort(A), be.token_sort(B)), A, B,
              "token_sort_ratio against indel of the sorted strings")


# ---- batch level ----

def batch_permutation(be, kind, m, A, B, k, seed):
    perm = list(range(len(A)))
    random.Random(seed).shuffle(perm)
    A2, B2 = [A[i] for i in perm], [B[i] for i in perm]
    same(kind, call(be, kind, m, A2, B2, k), call(be, kind, m, A, B, k)[perm], A2, B2, f"{m} {kind} k={k} with its rows permuted")


def batch_concatenation(be, kind, m, A1, B1, A2, B2, k):
    one = call(be, kind, m, A1 + A2, B1 + B2, k, role="mixed")
    two = np.concatenate([call(be, kind, m, A1, B1, k, role="base"), call(be, kind, m, A2, B2, k)])
    same(kind, one, two, A1 + A2, B1 + B2, f"{m} {kind} k={k} of two frames in one call")


def batch_literal(be, kind, m, X, lit, k):
    n = len(X)
    same(kind, call(be, kind, m, X, [lit], k), call(be, kind, m, X, [lit] * n, k), X, [lit], f"{m} {kind} k={k} literal on the right")
    same(kind, call(be, kind, m, [lit], X, k), call(be, kind, m, [lit] * n, X, k), [lit], X, f"{m} {kind} k={k} literal on the left")


# ---- searches ----

def search_invariance(be, entry, m, Q, Cs, Q2, Cs2, k, cut, what):
    """entry: "nearest" (cut = max_distance), "extract" (score_cutoff) or "best_match" (min_score)."""
    f = getattr(be, entry)
    same_lists(f(m, Q2, Cs2, k, cut, role="image"), f(m, Q, Cs, k, cut, role="base"), f"{entry} by {m} k={k} cutoff={cut} {what}")


# ---- backends ----

class ModelBackend:
    """The oracle for the classic five, the *_ref models for the rest (their C forms: the same recurrences, quick on long rows)."""

    def __init__(self):
        import best_match_ref
        import distance_ref
        import extract_ref
        import indel_ref
        import nearest_ref
        import oracle_lib
        import osa_ref
        import partial_ref
        import token_ref
        self.O, self.D, self.I, self.TK = oracle_lib, distance_ref, indel_ref, token_ref
        self.BM, self.NR, self.EX = best_match_ref, nearest_ref, extract_ref
        self.osa_c, self.indel_c, self.dist_c, self.partial_c = osa_ref.CRef(), indel_ref.CRef(), distance_ref.CDist(), partial_ref.CRef()

    def sim(self, m, A, B, role=None):
        A, B = bcast(A, B)
        if m in CLASSIC:
            return self.O.batch_strings(m, A, B, 4)
        if m == "osa":
            return np.array([self.osa_c.score(a, b) for a, b in zip(A, B)], dtype=np.float64)
        if m == "indel":
            return np.array([self.indel_c.score(a, b) for a, b in zip(A, B)], dtype=np.float64)
        if m == "partial_ratio":
            return self.partial_c.batch(A, B)[0]
        if m in TOKEN:  # (the model's rule pair by pair, its LCS from indel_ref's C form of the same recurrence)
            f = self.TK.token_sort_ratio if m == "token_sort_ratio" else self.TK.set_rule
            return np.array([f(a, b, self.indel_c.lcs) for a, b in zip(A, B)], dtype=np.float64)
        raise ValueError(m)

    def dist(self, m, A, B, k=None, role=None):
        A, B = bcast(A, B)
        if m == "indel":
            return self.I.clamp_array([self.indel_c.distance(a, b) for a, b in zip(A, B)], self.I.UNBOUNDED if k is None else k).astype(np.int64)
        return np.array([self.dist_c.distance(m, a, b, k) for a, b in zip(A, B)], dtype=np.int64)

    def partial(self, A, B, role=None):
        A, B = bcast(A, B)
        score, span, _, _ = self.partial_c.batch(A, B)
        return score, span.astype(np.int64)

    def token_sort(self, X, role=None):
        return [self.TK.token_sort(s) for s in X]

    def nearest(self, m, Q, Cs, k, md, role=None):
        return self.NR.topk(self.NR.distance_matrix(m, Q, Cs), k, md)

    def extract(self, scorer, Q, Cs, k, cutoff, role=None):
        return self.EX.extract("ratio" if scorer == "indel" else scorer, Q, Cs, k, cutoff)

    def best_match(self, m, Q, Cs, k, min_score, role=None):
        return self.BM.topk(self.BM.score_matrix(m, Q, Cs), k, min_score)


class GpuBackend:
    """strsim_amd.Context through its host entry points.  Every call is filed in `log` with the tier counters it left: the host calls
    end with the context's own synchronize(), so the counters are read right behind them."""

    def __init__(self, ctx):
        import strsim_amd
        self.S, self.ctx, self.log = strsim_amd, ctx, []

    def _file(self, entry, m, role, A, B):
        c = self.ctx
        self.log.append({"entry": entry, "measure": m, "role": role, "A": A, "B": B, "wave": c.last_wave_rows, "late": c.last_late_rows,
                         "long": c.last_long_rows, "token_wave": c.last_token_wave_rows if entry in ("sim", "token_sort") else 0})

    def sim(self, m, A, B, role=None):
        out = self.ctx.pairs_host(m, *self.S.pack_strings(A), *self.S.pack_strings(B))
        self._file("sim", m, role, A, B)
        return out

    def dist(self, m, A, B, k=None, role=None):
        out = self.ctx.distance_host(m, *self.S.pack_strings(A), *self.S.pack_strings(B), k).astype(np.int64)
        self._file("dist", m, role, A, B)
        return out

    def partial(self, A, B, role=None):
        score, span = self.ctx.partial_alignment_host(*self.S.pack_strings(A), *self.S.pack_strings(B))
        self._file("partial", "partial_ratio", role, A, B)
        return score, span.astype(np.int64)

    def token_sort(self, X, role=None):
        off, val = self.ctx.token_sort_host(*self.S.pack_strings(X))
        self.ctx.synchronize()
        self._file("token_sort", "token_sort", role, X, X)
        raw = val.tobytes()
        return [raw[int(off[i]):int(off[i + 1])].decode("utf-8") for i in range(len(X))]

    def _search(self, entry, m, Q, Cs, k, cut, role):
        idx, val = getattr(self.ctx, entry)(m, *self.S.pack_strings(Q), *self.S.pack_strings(Cs), k, cut)
        self._file(entry, m, role, Q, Cs)
        empty = idx == 0xFFFFFFFF
        assert np.array_equal(empty, np.isnan(val) if val.dtype == np.float64 else val == 0xFFFFFFFF)
        return np.where(empty, -1, idx.astype(np.int64)), (val if val.dtype == np.float64 else np.where(empty, -1, val.astype(np.int64)))

    def nearest(self, m, Q, Cs, k, md, role=None):
        return self._search("nearest", m, Q, Cs, k, md, role)

    def extract(self, scorer, Q, Cs, k, cutoff, role=None):
        return self._search("extract", scorer, Q, Cs, k, cutoff, role)

    def best_match(self, m, Q, Cs, k, min_score, role=None):
        return self._search("best_match", m, Q, Cs, k, min_score, role)
