"""Independent reference for the bounded edit distances (strsim_distance_device / _host): Levenshtein (measure 0) and optimal
string alignment (measure 6) over Unicode scalar values, with rapidfuzz's cutoff convention (d when d <= k, else k + 1; None is no
cutoff).

  * distance(measure, a, b, k): the textbook DP in plain Python;
  * batch_numpy(measure, A, B, k): the same recurrence vectorised over rows;
  * CDist: a rolling-row C DP built with the system C compiler, full or confined to a diagonal band (exact when the distance is
    within the band), for long strings.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

UNBOUNDED = 0xFFFFFFFF
MEASURE_ID = {"levenshtein": 0, "osa": 6}


def clamp(d, k):
    return d if k is None or k == UNBOUNDED or d <= k else k + 1


def distance(measure, a, b, k=None):
    tr = measure == "osa"
    la, lb = len(a), len(b)
    D = [[0] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        D[i][0] = i
    for j in range(lb + 1):
        D[0][j] = j
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            v = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
            if tr and i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                v = min(v, D[i - 2][j - 2] + 1)
            D[i][j] = v
    return clamp(D[la][lb], k)


def _codes(strings, L, pad):
    M = np.full((len(strings), max(L, 1)), pad, dtype=np.int64)
    for r, s in enumerate(strings):
        if s:
            M[r, :len(s)] = [ord(ch) for ch in s]
    return M


def batch_numpy(measure, A, B, k=None):
    """distance(measure, A[r], B[r], k) for every r (lists of str) -> uint32 array."""
    tr = measure == "osa"
    n = len(A)
    la = np.array([len(s) for s in A], dtype=np.int64)
    lb = np.array([len(s) for s in B], dtype=np.int64)
    La, Lb = int(la.max(initial=0)), int(lb.max(initial=0))
    X, Y = _codes(A, La, -1), _codes(B, Lb, -2)
    prev2 = None
    prev = np.broadcast_to(np.arange(Lb + 1, dtype=np.int64), (n, Lb + 1)).copy()
    d = prev[np.arange(n), lb].copy()
    for i in range(1, La + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        xi = X[:, i - 1]
        for j in range(1, Lb + 1):
            yj = Y[:, j - 1]
            v = np.minimum(np.minimum(prev[:, j] + 1, cur[:, j - 1] + 1), prev[:, j - 1] + (xi != yj))
            if tr and i > 1 and j > 1:
                t = (xi == Y[:, j - 2]) & (X[:, i - 2] == yj)
                v = np.where(t, np.minimum(v, prev2[:, j - 2] + 1), v)
            cur[:, j] = v
        hit = la == i
        d[hit] = cur[hit, lb[hit]]
        prev2, prev = prev, cur
    if k is not None and k != UNBOUNDED:
        d = np.minimum(d, k + 1)
    return d.astype(np.uint32)


_C_SRC = r"""
#include <stdint.h>
#include <stdlib.h>
/* edit distance with three rolling rows; tr = 1 adds the OSA transposition.  band: cells with |i - j| > band count as infinite
   (the result is exact when it is <= band; band >= max(la, lb) is the full DP). */
uint64_t dist_c(const uint32_t *a, uint64_t la, const uint32_t *b, uint64_t lb, int tr, uint64_t band)
{
    const uint64_t INF = (uint64_t)1 << 60;
    uint64_t *r0 = malloc((lb + 1) * 8), *r1 = malloc((lb + 1) * 8), *r2 = malloc((lb + 1) * 8);
    for (uint64_t j = 0; j <= lb; ++j) { r1[j] = j <= band ? j : INF; r0[j] = INF; }
    for (uint64_t i = 1; i <= la; ++i) {
        uint64_t j0 = i > band ? i - band : 1, j1 = i + band < lb ? i + band : lb;
        r2[0] = i <= band ? i : INF;
        if (j0 > 1) r2[j0 - 1] = INF;
        for (uint64_t j = j0; j <= j1; ++j) {
            uint64_t v = r1[j] + 1, w = r2[j - 1] + 1, s = r1[j - 1] + (a[i - 1] != b[j - 1]);
            if (w < v) v = w;
            if (s < v) v = s;
            if (tr && i > 1 && j > 1 && a[i - 1] == b[j - 2] && a[i - 2] == b[j - 1] && r0[j - 2] + 1 < v) v = r0[j - 2] + 1;
            r2[j] = v < INF ? v : INF;
        }
        if (j1 < lb) r2[j1 + 1] = INF;
        uint64_t *t = r0; r0 = r1; r1 = r2; r2 = t;
    }
    uint64_t d = r1[lb];
    free(r0); free(r1); free(r2);
    return d;
}
"""


class CDist:
    """The C DP, built once per instance into its own temp dir."""

    def __init__(self):
        self._dir = tempfile.TemporaryDirectory(prefix="dist_ref_")
        src = os.path.join(self._dir.name, "dist_ref.c")
        so = os.path.join(self._dir.name, "libdist_ref.so")
        with open(src, "w") as f:
            f.write(_C_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-o", so, src])
        self._L = C.CDLL(so)
        self._L.dist_c.restype = C.c_uint64
        self._L.dist_c.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64]

    def distance(self, measure, a, b, k=None, band=None):
        """band: confine the DP to |i - j| <= band -- then the result is exact only when it is <= band (None: the full DP)."""
        x = np.array([ord(c) for c in a] or [0], dtype=np.uint32)
        y = np.array([ord(c) for c in b] or [0], dtype=np.uint32)
        full = max(len(a), len(b))
        d = int(self._L.dist_c(x.ctypes.data, len(a), y.ctypes.data, len(b), 1 if measure == "osa" else 0,
                               full if band is None else min(band, full)))
        if band is not None and d > band:
            raise ValueError("the distance is beyond the band: no exact answer")
        return clamp(d, k)


# Known answers: (a, b, levenshtein, osa)
KNOWN = [
    ("kitten", "sitting", 3, 3),
    ("abcd", "acbd", 2, 1),
    ("ca", "abc", 3, 3),
    ("", "héllo", 5, 5),
    ("héllo", "", 5, 5),
    ("", "", 0, 0),
    ("東京都", "京東都", 2, 1),
    ("日本語の文章", "日本語文章", 1, 1),
    ("😀😃😄", "😃😀😄", 2, 1),
    ("a😀b𝄞", "a😀c𝄞", 1, 1),
    ("jonh", "john", 2, 1),
]
