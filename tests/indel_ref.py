"""Independent reference for the Indel (longest-common-subsequence) similarity and distance, measure id 8.

Three forms of the textbook LCS DP, held to each other by tests/test_indel_cpu.py:
  * lcs(a, b): plain Python over `str` (Unicode scalar values);
  * batch_numpy_lcs(A, B): the same recurrence vectorised over rows, for frames of a few hundred thousand short rows;
  * CRef: a textbook rolling-row C DP compiled with the system C compiler into a temp dir, for long strings.
distance = |a| + |b| - 2 lcs (insertions and deletions only: a substitution costs 2).  normalise() is the library's score, with
exactly two f64 operations: 1.0 when |a| + |b| == 0, else 1.0 - (d / (|a| + |b|)) -- rapidfuzz's Indel.normalized_similarity,
fuzz.ratio / 100.  It is NOT 2 lcs / (|a| + |b|): the two differ in the last bit for many (lcs, |a| + |b|).
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

UNBOUNDED = 0xFFFFFFFF


def lcs(a: str, b: str) -> int:
    la, lb = len(a), len(b)
    D = [[0] * (lb + 1) for _ in range(la + 1)]
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            D[i][j] = D[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(D[i - 1][j], D[i][j - 1])
    return D[la][lb]


def distance(a: str, b: str) -> int:
    return len(a) + len(b) - 2 * lcs(a, b)


def clamp(d: int, k: int) -> int:
    """The distance call's output for cutoff k (UNBOUNDED: none): d when d <= k, else k + 1."""
    return d if k == UNBOUNDED or d <= k else k + 1


def normalise(d: int, la: int, lb: int) -> float:
    if la + lb == 0:
        return 1.0
    return 1.0 - (float(d) / float(la + lb))


def score(a: str, b: str) -> float:
    return normalise(distance(a, b), len(a), len(b))


def _codes(strings, L, pad):
    M = np.full((len(strings), max(L, 1)), pad, dtype=np.int64)
    for r, s in enumerate(strings):
        if s:
            M[r, :len(s)] = [ord(ch) for ch in s]
    return M


def batch_numpy_lcs(A, B):
    """lcs(A[r], B[r]) for every r (lists of str), vectorised over rows -> int64."""
    n = len(A)
    la = np.array([len(s) for s in A], dtype=np.int64)
    lb = np.array([len(s) for s in B], dtype=np.int64)
    La, Lb = int(la.max(initial=0)), int(lb.max(initial=0))
    X, Y = _codes(A, La, -1), _codes(B, Lb, -2)  # (the pads never match: cells past a string's end repeat the last real one)
    prev = np.zeros((n, Lb + 1), dtype=np.int64)
    for i in range(1, La + 1):
        cur = np.zeros_like(prev)
        xi = X[:, i - 1]
        for j in range(1, Lb + 1):
            cur[:, j] = np.where(xi == Y[:, j - 1], prev[:, j - 1] + 1, np.maximum(prev[:, j], cur[:, j - 1]))
        prev = cur
    return prev[:, Lb].copy() if n else np.zeros(0, dtype=np.int64)


def batch_numpy_distance(A, B):
    la = np.array([len(s) for s in A], dtype=np.int64)
    lb = np.array([len(s) for s in B], dtype=np.int64)
    return la + lb - 2 * batch_numpy_lcs(A, B)


def scores_from_distances(d, la, lb):
    """normalise() over arrays: the same two f64 operations (numpy's f64 division and subtraction are IEEE ones)."""
    d = np.asarray(d, dtype=np.int64)
    den = (np.asarray(la, dtype=np.int64) + np.asarray(lb, dtype=np.int64)).astype(np.float64)
    out = np.empty(d.size, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:] = 1.0 - (d.astype(np.float64) / den)
    out[den == 0.0] = 1.0
    return out


def batch_numpy(A, B):
    """score(A[r], B[r]) for every r."""
    return scores_from_distances(batch_numpy_distance(A, B), [len(s) for s in A], [len(s) for s in B])


def clamp_array(d, k):
    d = np.asarray(d, dtype=np.int64)
    if k == UNBOUNDED:
        return d.astype(np.uint32)
    return np.where(d <= k, d, k + 1).astype(np.uint32)


_C_SRC = r"""
#include <stdint.h>
#include <stdlib.h>
/* textbook LCS length with two rolling rows */
uint64_t indel_c_lcs(const uint32_t *a, uint64_t la, const uint32_t *b, uint64_t lb)
{
    uint32_t *r0 = calloc(lb + 1, 4), *r1 = calloc(lb + 1, 4);
    for (uint64_t i = 1; i <= la; ++i) {
        r1[0] = 0;
        for (uint64_t j = 1; j <= lb; ++j) {
            if (a[i - 1] == b[j - 1]) r1[j] = r0[j - 1] + 1;
            else r1[j] = r0[j] > r1[j - 1] ? r0[j] : r1[j - 1];
        }
        uint32_t *t = r0; r0 = r1; r1 = t;
    }
    uint64_t l = r0[lb];
    free(r0); free(r1);
    return l;
}
"""


class CRef:
    """The C DP, built once per instance into its own temp dir."""

    def __init__(self):
        self._dir = tempfile.TemporaryDirectory(prefix="indel_ref_")
        src = os.path.join(self._dir.name, "indel_ref.c")
        so = os.path.join(self._dir.name, "libindel_ref.so")
        with open(src, "w") as f:
            f.write(_C_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-o", so, src])
        self._L = C.CDLL(so)
        self._L.indel_c_lcs.restype = C.c_uint64
        self._L.indel_c_lcs.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]

    def lcs(self, a: str, b: str) -> int:
        x = np.array([ord(c) for c in a] or [0], dtype=np.uint32)
        y = np.array([ord(c) for c in b] or [0], dtype=np.uint32)
        return int(self._L.indel_c_lcs(x.ctypes.data, len(a), y.ctypes.data, len(b)))

    def distance(self, a: str, b: str) -> int:
        return len(a) + len(b) - 2 * self.lcs(a, b)

    def score(self, a: str, b: str) -> float:
        return normalise(self.distance(a, b), len(a), len(b))


def mixed_distances(A, B, cref, short=24):
    """Distances of a frame with a few long rows: the numpy form for rows of up to `short` characters, the C DP for the rest."""
    d = np.zeros(len(A), dtype=np.int64)
    small = [r for r in range(len(A)) if len(A[r]) <= short and len(B[r]) <= short]
    if small:
        d[small] = batch_numpy_distance([A[r] for r in small], [B[r] for r in small])
    sm = set(small)
    for r in range(len(A)):
        if r not in sm:
            d[r] = cref.distance(A[r], B[r])
    return d


# The issue's known answers: (a, b, lcs, d); the score follows from normalise()
KNOWN = [
    ("ab", "ba", 1, 2),
    ("jonh", "john", 3, 2),
    ("martha", "marhta", 5, 2),
    ("kitten", "sitting", 4, 5),
    ("phillips", "philips", 7, 1),
    ("dixon", "dicksonx", 4, 5),
    ("müller", "mülelr", 5, 2),
    ("abc", "xyz", 0, 6),
    ("", "abc", 0, 3),
    ("", "", 0, 0),
    ("a" * 63 + "xy", "a" * 63 + "yx", 64, 2),
]
KNOWN_SCORES = {("ab", "ba"): 0.5, ("jonh", "john"): 0.75, ("abc", "xyz"): 0.0, ("", "abc"): 0.0, ("", ""): 1.0}
