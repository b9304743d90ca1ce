"""Independent reference for the unrestricted Damerau-Levenshtein distance (strsim_damerau_*).

Two forms of the Lowrance-Wagner FULL-MATRIX DP -- deliberately not the linear-space form the kernels run -- held to each other and
to a search over single edits by tests/test_damerau_cpu.py:
  * distance(a, b): plain Python over `str` (Unicode scalar values);
  * CRef: the same DP in C, compiled with the system C compiler into a temp dir, for long strings.  Its table of the last row of
    every character has 0x110000 entries, of which only the touched ones are reset.
score(a, b) is the normalisation the library uses: 1.0 when a == b or both are empty, else 1.0 - d / max(|a|, |b|).
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np


def distance(a: str, b: str) -> int:
    la, lb = len(a), len(b)
    big = la + lb
    # H[i + 1][j + 1] = D[i][j]; row and column 0 of H hold `big`
    H = [[big] * (lb + 2) for _ in range(la + 2)]
    for i in range(la + 1):
        H[i + 1][1] = i
    for j in range(lb + 1):
        H[1][j + 1] = j
    last_row = {}
    for i in range(1, la + 1):
        last_col = 0
        for j in range(1, lb + 1):
            k = last_row.get(b[j - 1], 0)
            l = last_col
            cost = 1
            if a[i - 1] == b[j - 1]:
                cost = 0
                last_col = j
            H[i + 1][j + 1] = min(H[i][j] + cost, H[i + 1][j] + 1, H[i][j + 1] + 1, H[k][l] + (i - k - 1) + 1 + (j - l - 1))
        last_row[a[i - 1]] = i
    return H[la + 1][lb + 1]


def normalise(d: int, la: int, lb: int) -> float:
    if la == 0 and lb == 0:
        return 1.0
    return 1.0 - (float(d) / float(max(la, lb)))


def score(a: str, b: str) -> float:
    if a == b:
        return 1.0
    return normalise(distance(a, b), len(a), len(b))


_C_SRC = r"""
#include <stdint.h>
#include <stdlib.h>
static uint64_t last_row[0x110000];
/* Lowrance-Wagner, the whole (la + 2) x (lb + 2) matrix */
uint64_t dl_c_distance(const uint32_t *a, uint64_t la, const uint32_t *b, uint64_t lb)
{
    const uint64_t W = lb + 2, big = la + lb; /* (distances fit 32 bits: 4 bytes a cell keep 5 000 x 5 000 at 100 MB) */
    uint32_t *H = malloc((la + 2) * W * 4);
    for (uint64_t j = 0; j < W; ++j) H[j] = big;
    for (uint64_t i = 0; i <= la; ++i) { H[(i + 1) * W] = big; H[(i + 1) * W + 1] = i; }
    for (uint64_t j = 0; j <= lb; ++j) H[W + j + 1] = j;
    for (uint64_t i = 1; i <= la; ++i) {
        uint64_t last_col = 0;
        for (uint64_t j = 1; j <= lb; ++j) {
            const uint64_t k = last_row[b[j - 1]], l = last_col;
            uint64_t cost = 1;
            if (a[i - 1] == b[j - 1]) { cost = 0; last_col = j; }
            uint64_t v = H[i * W + j] + cost;
            const uint64_t w = H[(i + 1) * W + j] + 1, u = H[i * W + j + 1] + 1, t = H[k * W + l] + (i - k - 1) + 1 + (j - l - 1);
            if (w < v) v = w;
            if (u < v) v = u;
            if (t < v) v = t;
            H[(i + 1) * W + j + 1] = v;
        }
        last_row[a[i - 1]] = i;
    }
    const uint64_t d = H[(la + 1) * W + lb + 1];
    for (uint64_t i = 0; i < la; ++i) last_row[a[i]] = 0;
    free(H);
    return d;
}
"""


class CRef:
    """The C DP, built once per instance into its own temp dir."""

    def __init__(self):
        self._dir = tempfile.TemporaryDirectory(prefix="damerau_ref_")
        src = os.path.join(self._dir.name, "damerau_ref.c")
        so = os.path.join(self._dir.name, "libdamerau_ref.so")
        with open(src, "w") as f:
            f.write(_C_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-o", so, src])
        self._L = C.CDLL(so)
        self._L.dl_c_distance.restype = C.c_uint64
        self._L.dl_c_distance.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]

    def distance(self, a: str, b: str) -> int:
        x = np.array([ord(c) for c in a] or [0], dtype=np.uint32)
        y = np.array([ord(c) for c in b] or [0], dtype=np.uint32)
        return int(self._L.dl_c_distance(x.ctypes.data, len(a), y.ctypes.data, len(b)))

    def score(self, a: str, b: str) -> float:
        if a == b:
            return 1.0
        return normalise(self.distance(a, b), len(a), len(b))

    def distances(self, A, B):
        """uint32 array of the distances of two columns, one of which may be a literal (one row)"""
        n = max(len(A), len(B))
        A = list(A) * n if len(A) == 1 else A
        B = list(B) * n if len(B) == 1 else B
        return np.array([self.distance(a, b) for a, b in zip(A, B)], dtype=np.uint32)

    def scores(self, A, B):
        n = max(len(A), len(B))
        A = list(A) * n if len(A) == 1 else A
        B = list(B) * n if len(B) == 1 else B
        return np.array([self.score(a, b) for a, b in zip(A, B)], dtype=np.float64)


def clamp(d, k):
    """what a distance call with max_distance=k returns for the distances d (k None: no cutoff)"""
    d = np.asarray(d, dtype=np.uint32)
    return d if k is None else np.minimum(d.astype(np.int64), k + 1).astype(np.uint32)


# The issue's known answers: (a, b, d, d_osa)
KNOWN = [
    ("ca", "abc", 2, 3),
    ("cä", "äbc", 2, 3),
    ("a cat", "an abct", 3, 4),
    ("ab", "ba", 1, 1),
    ("jonh", "john", 1, 1),
    ("abcdef", "badcfe", 3, 3),
    ("dixon", "dicksonx", 4, 4),
    ("", "abc", 3, 3),
    ("", "", 0, 0),
    ("x" * 40 + "ca", "x" * 40 + "abc", 2, 3),
    ("a" * 63 + "xy", "a" * 63 + "yzx", 2, 3),
    ("é" * 63 + "xy", "é" * 63 + "yzx", 2, 3),
]
# and the scores the issue states
KNOWN_SCORES = [
    ("cä", "äbc", 0.33333333333333337),
    ("x" * 40 + "ca", "x" * 40 + "abc", 0.9534883720930233),
    ("a" * 63 + "xy", "a" * 63 + "yzx", 0.9696969696969697),
    ("é" * 63 + "xy", "é" * 63 + "yzx", 0.9696969696969697),
]


# ---- generators ----

def swapped(rng, s, k):
    """s with k random swaps of two adjacent characters"""
    c = list(s)
    for _ in range(k):
        if len(c) < 2:
            break
        i = rng.randrange(len(c) - 1)
        c[i], c[i + 1] = c[i + 1], c[i]
    return "".join(c)


def gapped(rng, s, k, alphabet):
    """s where k times an adjacent x y became y z x with a random z: the edit the restricted distance cannot see as 2"""
    c = list(s)
    for _ in range(k):
        if len(c) < 2:
            break
        i = rng.randrange(len(c) - 1)
        c[i:i + 2] = [c[i + 1], rng.choice(alphabet), c[i]]
    return "".join(c)


def gapped_at(s, i, z):
    """s with the x y at positions i, i + 1 (0-based) turned into y z x"""
    return s[:i] + s[i + 1] + z + s[i] + s[i + 2:]


LOWER = "abcdefghijklmnopqrstuvwxyz"


def lane_frame(rng, n, lane_max):
    """The GPU lane frame: lowercase rows of 0 .. lane_max characters, b a gapped / swapped / truncated a that still fits."""
    A, B = [], []
    for r in range(n):
        la = rng.randrange(lane_max + 1)
        a = "".join(rng.choice(LOWER) for _ in range(la))
        kind = r % 4
        if kind == 0:
            b = gapped(rng, a, rng.randrange(1, 4), LOWER)
        elif kind == 1:
            b = swapped(rng, a, rng.randrange(1, 4))
        elif kind == 2:
            b = gapped(rng, a[:rng.randrange(la + 1)], 1, LOWER)
        else:
            b = swapped(rng, gapped(rng, a, 1, LOWER), 1)
        A.append(a)
        B.append(b[:lane_max])
    return A, B
