"""Independent model of token_ratio, partial_token_sort_ratio, partial_token_set_ratio, partial_token_ratio and wratio (measure
ids 18, 20, 22, 24 and 26): rapidfuzz's fuzz.token_ratio, fuzz.partial_token_sort_ratio, fuzz.partial_token_set_ratio,
fuzz.partial_token_ratio and fuzz.WRatio, each / 100, without a processor.

Everything is composed from the models of the measures below them: indel and the token forms from token_ref (textbook LCS), the
partial ratio from partial_ref (brute force over every window).  Lengths are Python's len(): Unicode scalar values.

  token_ratio(a, b)               max(token_sort_ratio, token_set_ratio)
  partial_token_sort_ratio(a, b)  partial_ratio(token_sort(a), token_sort(b))
  partial_token_set_ratio(a, b)   0.0 when A or B is empty, 1.0 when A & B is not, else partial_ratio(ab, ba)
  partial_token_ratio(a, b)       max(partial_token_sort_ratio, partial_token_set_ratio)
  wratio(a, b)                    lo, hi = min, max of len(a), len(b); r = indel(a, b)
                                  0.0 when lo == 0
                                  near (2 hi < 3 lo):  max(r, token_ratio * 0.95)
                                  far:                 ps = 0.9 when hi <= 8 lo else 0.6
                                                       max(r, partial_ratio * ps, (partial_token_ratio * 0.95) * ps)

partial_token_ratio_rapidfuzz is a transcription of rapidfuzz's own early-exit form (fuzz_py.partial_token_ratio), which
tests/test_wratio_cpu.py holds the max() form to.  The two differ for strings without tokens alone (rapidfuzz: 0, the max() form:
1.0 for two of them), where wratio is 0.0 before it gets there.

Frames evaluates whole frames (lists of str) with the C forms of the two brute forces (indel_ref.CRef, partial_ref.CRef).
"""
import numpy as np

import indel_ref
import partial_ref
import token_ref as T

IDS = {"token_ratio": 18, "partial_token_sort_ratio": 20, "partial_token_set_ratio": 22, "partial_token_ratio": 24, "wratio": 26}
EMPTY, NEAR, FAR8, FAR = 0, 1, 2, 3


def partial_ratio(a: str, b: str) -> float:
    return partial_ref.partial(a, b)[0]


def token_ratio(a: str, b: str) -> float:
    return max(T.token_sort_ratio(a, b), T.token_set_ratio(a, b))


def partial_token_sort_ratio(a: str, b: str, partial=partial_ratio) -> float:
    return partial(T.token_sort(a), T.token_sort(b))


def partial_token_set_ratio(a: str, b: str, partial=partial_ratio) -> float:
    A, B = set(T.tokens(a)), set(T.tokens(b))
    if not A or not B:
        return 0.0
    if A & B:
        return 1.0
    _, ab, ba = T.set_parts(a, b)
    return partial(ab, ba)


def partial_token_ratio(a: str, b: str, partial=partial_ratio) -> float:
    return max(partial_token_sort_ratio(a, b, partial), partial_token_set_ratio(a, b, partial))


def partial_token_ratio_rapidfuzz(a: str, b: str, partial=partial_ratio) -> float:
    """rapidfuzz's fuzz_py.partial_token_ratio, line by line, in [0, 1]."""
    tokens_split_a = a.split()
    tokens_split_b = b.split()
    tokens_a = set(tokens_split_a)
    tokens_b = set(tokens_split_b)
    if not tokens_a or not tokens_b:
        return 0.0
    # exit early when there is a common word in both sequences
    if tokens_a.intersection(tokens_b):
        return 1.0
    diff_ab = tokens_a.difference(tokens_b)
    diff_ba = tokens_b.difference(tokens_a)
    result = partial(" ".join(sorted(tokens_split_a)), " ".join(sorted(tokens_split_b)))
    # do not calculate the same partial_ratio twice
    if len(tokens_split_a) == len(diff_ab) and len(tokens_split_b) == len(diff_ba):
        return result
    return max(result, partial(" ".join(sorted(diff_ab)), " ".join(sorted(diff_ba))))


def wratio_class(la: int, lb: int) -> int:
    lo, hi = min(la, lb), max(la, lb)
    if lo == 0:
        return EMPTY
    if 2 * hi < 3 * lo:
        return NEAR
    return FAR8 if hi <= 8 * lo else FAR


def wratio_rule(cls: int, r: float, s0: float, s1: float) -> float:
    """near: s0 = token_ratio; far: s0 = partial_ratio, s1 = partial_token_ratio."""
    if cls == EMPTY:
        return 0.0
    if cls == NEAR:
        return max(r, s0 * 0.95)
    ps = 0.9 if cls == FAR8 else 0.6
    return max(r, s0 * ps, (s1 * 0.95) * ps)


def wratio(a: str, b: str) -> float:
    cls = wratio_class(len(a), len(b))
    if cls == EMPTY:
        return 0.0
    r = T.indel(a, b)
    if cls == NEAR:
        return wratio_rule(cls, r, token_ratio(a, b), 0.0)
    return wratio_rule(cls, r, partial_ratio(a, b), partial_token_ratio(a, b))


SCORE = {"token_ratio": token_ratio, "partial_token_sort_ratio": partial_token_sort_ratio,
         "partial_token_set_ratio": partial_token_set_ratio, "partial_token_ratio": partial_token_ratio, "wratio": wratio}


class Frames:
    """The same definitions over lists of str, with the C brute forces.  columns(A, B) -> {name: f64 array} for the four measures
    the five are built from and the five themselves, plus "class" (the wratio class of each row, uint8)."""

    def __init__(self):
        self.ic = indel_ref.CRef()
        self.pc = partial_ref.CRef()

    def indel(self, A, B):
        return np.array([T.indel(a, b, self.ic.lcs) for a, b in zip(A, B)], dtype=np.float64)

    def partial(self, A, B):
        return self.pc.batch(list(A), list(B))[0]

    def columns(self, A, B):
        A, B = T.broadcast(list(A), list(B))
        n = len(A)
        SA, SB = [T.token_sort(s) for s in A], [T.token_sort(s) for s in B]
        parts = [T.set_parts(a, b) for a, b in zip(A, B)]
        c = {}
        c["indel"] = self.indel(A, B)
        c["partial_ratio"] = self.partial(A, B)
        c["token_sort_ratio"] = self.indel(SA, SB)
        c["token_set_ratio"] = np.array([T.set_rule(a, b, self.ic.lcs) for a, b in zip(A, B)], dtype=np.float64)
        c["token_ratio"] = np.maximum(c["token_sort_ratio"], c["token_set_ratio"])
        c["partial_token_sort_ratio"] = self.partial(SA, SB)
        pset = self.partial([p[1] for p in parts], [p[2] for p in parts])
        for i in range(n):
            if not T.tokens(A[i]) or not T.tokens(B[i]):
                pset[i] = 0.0
            elif parts[i][0]:
                pset[i] = 1.0
        c["partial_token_set_ratio"] = pset
        c["partial_token_ratio"] = np.maximum(c["partial_token_sort_ratio"], pset)
        cls = np.array([wratio_class(len(a), len(b)) for a, b in zip(A, B)], dtype=np.uint8)
        c["class"] = cls
        c["wratio"] = combine(cls, c["indel"], c["token_ratio"], c["partial_ratio"], c["partial_token_ratio"])
        return c


def combine(cls, r, token_ratio_col, partial_col, partial_token_col):
    """wratio_rule over arrays, row by row in Python floats (IEEE f64 products in the rule's association)."""
    out = np.empty(len(cls), dtype=np.float64)
    for i in range(len(cls)):
        k = int(cls[i])
        if k == NEAR:
            out[i] = wratio_rule(k, float(r[i]), float(token_ratio_col[i]), 0.0)
        else:
            out[i] = wratio_rule(k, float(r[i]), float(partial_col[i]), float(partial_token_col[i]))
    return out
