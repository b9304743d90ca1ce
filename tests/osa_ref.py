"""Independent reference for optimal string alignment (restricted Damerau-Levenshtein), measure id 6.

Three forms of the textbook DP, held to each other by tests/test_osa_cpu.py:
  * distance(a, b): plain Python over `str` (Unicode scalar values);
  * batch_numpy(A, B): the same recurrence vectorised over rows, for frames of a few hundred thousand short rows;
  * CRef: a textbook rolling-row C DP compiled with the system C compiler into a temp dir, for long strings.
score(a, b) is the normalisation the library uses: 1.0 when a == b or both are empty, else 1.0 - d / max(|a|, |b|).
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np


def distance(a: str, b: str) -> int:
    la, lb = len(a), len(b)
    D = [[0] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        D[i][0] = i
    for j in range(lb + 1):
        D[0][j] = j
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            cost = 0 if a[i - 1] == b[j - 1] else 1
            v = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + cost)
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                v = min(v, D[i - 2][j - 2] + 1)
            D[i][j] = v
    return D[la][lb]


def normalise(d: int, la: int, lb: int) -> float:
    if la == 0 and lb == 0:
        return 1.0
    return 1.0 - (float(d) / float(max(la, lb)))


def score(a: str, b: str) -> float:
    if a == b:
        return 1.0
    return normalise(distance(a, b), len(a), len(b))


def _codes(strings, L, pad):
    M = np.full((len(strings), max(L, 1)), pad, dtype=np.int64)
    for r, s in enumerate(strings):
        if s:
            M[r, :len(s)] = [ord(ch) for ch in s]
    return M


def batch_numpy(A, B):
    """score(A[r], B[r]) for every r (lists of str), vectorised over rows."""
    n = len(A)
    la = np.array([len(s) for s in A], dtype=np.int64)
    lb = np.array([len(s) for s in B], dtype=np.int64)
    La, Lb = int(la.max(initial=0)), int(lb.max(initial=0))
    X, Y = _codes(A, La, -1), _codes(B, Lb, -2)
    cols = np.arange(Lb + 1, dtype=np.int64)
    prev2 = None
    prev = np.broadcast_to(cols, (n, Lb + 1)).copy()           # row i = 0
    d = prev[np.arange(n), lb].copy()                           # rows with la == 0
    for i in range(1, La + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        xi = X[:, i - 1]
        for j in range(1, Lb + 1):
            yj = Y[:, j - 1]
            v = np.minimum(np.minimum(prev[:, j] + 1, cur[:, j - 1] + 1), prev[:, j - 1] + (xi != yj))
            if i > 1 and j > 1:
                tr = (xi == Y[:, j - 2]) & (X[:, i - 2] == yj)
                v = np.where(tr, np.minimum(v, prev2[:, j - 2] + 1), v)
            cur[:, j] = v
        hit = la == i
        d[hit] = cur[hit, lb[hit]]
        prev2, prev = prev, cur
    out = np.empty(n, dtype=np.float64)
    both_empty = (la == 0) & (lb == 0)
    den = np.maximum(la, lb).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:] = 1.0 - (d.astype(np.float64) / den)
    out[both_empty] = 1.0
    return out


_C_SRC = r"""
#include <stdint.h>
#include <stdlib.h>
/* textbook OSA distance with three rolling rows (i - 2, i - 1, i) */
uint64_t osa_c_distance(const uint32_t *a, uint64_t la, const uint32_t *b, uint64_t lb)
{
    uint64_t *r0 = malloc((lb + 1) * 8), *r1 = malloc((lb + 1) * 8), *r2 = malloc((lb + 1) * 8);
    for (uint64_t j = 0; j <= lb; ++j) r1[j] = j;
    for (uint64_t i = 1; i <= la; ++i) {
        r2[0] = i;
        for (uint64_t j = 1; j <= lb; ++j) {
            uint64_t v = r1[j] + 1, w = r2[j - 1] + 1, s = r1[j - 1] + (a[i - 1] != b[j - 1]);
            if (w < v) v = w;
            if (s < v) v = s;
            if (i > 1 && j > 1 && a[i - 1] == b[j - 2] && a[i - 2] == b[j - 1] && r0[j - 2] + 1 < v) v = r0[j - 2] + 1;
            r2[j] = v;
        }
        uint64_t *t = r0; r0 = r1; r1 = r2; r2 = t;
    }
    uint64_t d = r1[lb];
    free(r0); free(r1); free(r2);
    return d;
}
"""


class CRef:
    """The C DP, built once per instance into its own temp dir."""

    def __init__(self):
        self._dir = tempfile.TemporaryDirectory(prefix="osa_ref_")
        src = os.path.join(self._dir.name, "osa_ref.c")
        so = os.path.join(self._dir.name, "libosa_ref.so")
        with open(src, "w") as f:
            f.write(_C_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-o", so, src])
        self._L = C.CDLL(so)
        self._L.osa_c_distance.restype = C.c_uint64
        self._L.osa_c_distance.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]

    def distance(self, a: str, b: str) -> int:
        x = np.array([ord(c) for c in a] or [0], dtype=np.uint32)
        y = np.array([ord(c) for c in b] or [0], dtype=np.uint32)
        return int(self._L.osa_c_distance(x.ctypes.data, len(a), y.ctypes.data, len(b)))

    def score(self, a: str, b: str) -> float:
        if a == b:
            return 1.0
        return normalise(self.distance(a, b), len(a), len(b))


# The issue's known answers: (a, b, d_osa, d_lev, score)
KNOWN = [
    ("ab", "ba", 1, 2, 0.5),
    ("ca", "abc", 3, 3, 0.0),
    ("jonh", "john", 1, 2, 0.75),
    ("martha", "marhta", 1, 2, 0.8333333333333334),
    ("abcdef", "badcfe", 3, 4, 0.5),
    ("müller", "mülelr", 1, 2, 0.8333333333333334),
    ("phillips", "philips", 1, 1, 0.875),
    ("dixon", "dicksonx", 4, 4, 0.5),
    ("", "phillips", 8, 8, 0.0),
    ("", "", 0, 0, 1.0),
    ("a" * 63 + "xy", "a" * 63 + "yx", 1, 2, 0.9846153846153847),
]
