"""Independent model of the partial ratio (best-window Indel similarity) and its alignment, measure id 10.

For a needle s (m = len(s) >= 1) and a haystack t (n = len(t) >= m) the windows of t are, in the tie order,
  * the proper prefixes t[0:w], w = 1 .. m-1,
  * every substring of length m, t[i:i+m], i = 0 .. n-m,
  * the proper suffixes t[i:n], i = n-m+1 .. n-1
(n + m - 1 windows: smallest end first, then smallest start).  P(s, t) is the maximum of indel_ref.score(s, window) over them, the
first strict maximum winning.  partial(a, b): both empty -> 1.0, one empty -> 0.0, the shorter string is the needle, and for equal
lengths a is the needle unless b as the needle scores strictly higher.  Everything is brute force: every window is scored by the
textbook LCS DP of indel_ref.  A C form of the same brute force (CRef) serves frames of 10^5 rows.  Nothing here shares code with
the library.  This is rapidfuzz's fuzz.partial_ratio / 100 for needles of up to 64 characters as its sources describe it; beyond
that rapidfuzz uses a heuristic and this model (and the library) keep the maximum.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import indel_ref


def windows(m: int, n: int):
    """(start, end) of every window of a haystack of n against a needle of m (1 <= m <= n), in the tie order."""
    out = [(0, w) for w in range(1, m)]
    out += [(i, i + m) for i in range(0, n - m + 1)]
    out += [(i, n) for i in range(n - m + 1, n)]
    return out


def _P(s: str, t: str):
    best = None
    for (i, e) in windows(len(s), len(t)):
        sc = indel_ref.score(s, t[i:e])
        if best is None or sc > best[0]:
            best = (sc, i, e)
    return best


def partial(a: str, b: str):
    """(score, a_start, a_end, b_start, b_end)."""
    la, lb = len(a), len(b)
    if la == 0 or lb == 0:
        return (1.0 if la == lb else 0.0, 0, 0, 0, 0)
    if la < lb:
        sc, i, e = _P(a, b)
        return (sc, 0, la, i, e)
    if la > lb:
        sc, i, e = _P(b, a)
        return (sc, i, e, 0, lb)
    s1, i1, e1 = _P(a, b)
    s2, i2, e2 = _P(b, a)
    if s2 > s1:
        return (s2, i2, e2, 0, lb)
    return (s1, 0, la, i1, e1)


def count_at_max(a: str, b: str) -> int:
    """How many windows (of the winning direction) reach the maximum: > 1 means the tie rule decided the span."""
    if not a or not b:
        return 1
    sc = partial(a, b)[0]
    a_needle = len(a) < len(b) or (len(a) == len(b) and not second_direction_wins(a, b))
    s, t = (a, b) if a_needle else (b, a)
    return sum(1 for (i, e) in windows(len(s), len(t)) if indel_ref.score(s, t[i:e]) == sc)


def second_direction_wins(a: str, b: str) -> bool:
    """len(a) == len(b) and P(b, a) > P(a, b)."""
    return len(a) == len(b) and len(a) > 0 and _P(b, a)[0] > _P(a, b)[0]


_C_SRC = r"""
#include <stdint.h>
#include <stdlib.h>
static uint32_t lcs(const uint32_t *a, uint32_t la, const uint32_t *b, uint32_t lb, uint32_t *r0, uint32_t *r1)
{
    for (uint32_t j = 0; j <= lb; ++j) r0[j] = 0;
    for (uint32_t i = 1; i <= la; ++i) {
        r1[0] = 0;
        for (uint32_t j = 1; j <= lb; ++j) {
            if (a[i - 1] == b[j - 1]) r1[j] = r0[j - 1] + 1;
            else r1[j] = r0[j] > r1[j - 1] ? r0[j] : r1[j - 1];
        }
        uint32_t *t = r0; r0 = r1; r1 = t;
    }
    return r0[lb];
}
static double score(uint32_t l, uint32_t m, uint32_t w)
{
    if (m + w == 0) return 1.0;
    return 1.0 - ((double)(m + w - 2 * l) / (double)(m + w));
}
/* best window of t (n values) against s (m values), 1 <= m <= n, windows in the tie order, first strict maximum */
static double P(const uint32_t *s, uint32_t m, const uint32_t *t, uint32_t n, uint32_t *ws, uint32_t *we, uint32_t *ties,
                uint32_t *r0, uint32_t *r1)
{
    double best = -1.0;
    uint32_t cnt = 0;
    for (uint32_t k = 0; k < n + m - 1; ++k) {
        uint32_t i, e;
        if (k < m - 1) { i = 0; e = k + 1; }
        else if (k < n) { i = k - (m - 1); e = i + m; }
        else { i = k - (m - 1); e = n; }
        const double sc = score(lcs(s, m, t + i, e - i, r0, r1), m, e - i);
        if (sc > best) { best = sc; *ws = i; *we = e; cnt = 1; }
        else if (sc == best) ++cnt;
    }
    *ties = cnt;
    return best;
}
/* out5: a_start, a_end, b_start, b_end, windows at the maximum (of the winning direction); flag: 1 when |a| == |b| and b as the
   needle is strictly better */
double partial_c(const uint32_t *a, uint32_t la, const uint32_t *b, uint32_t lb, uint32_t *out5, uint32_t *flag)
{
    out5[0] = out5[1] = out5[2] = out5[3] = 0; out5[4] = 1; *flag = 0;
    if (la == 0 || lb == 0) return la == lb ? 1.0 : 0.0;
    const uint32_t n = la > lb ? la : lb;
    uint32_t *r0 = malloc((n + 1) * 4), *r1 = malloc((n + 1) * 4);
    uint32_t ws, we, ties;
    double sc;
    if (la < lb) { sc = P(a, la, b, lb, &ws, &we, &ties, r0, r1); out5[0] = 0; out5[1] = la; out5[2] = ws; out5[3] = we; out5[4] = ties; }
    else if (la > lb) { sc = P(b, lb, a, la, &ws, &we, &ties, r0, r1); out5[0] = ws; out5[1] = we; out5[2] = 0; out5[3] = lb; out5[4] = ties; }
    else {
        sc = P(a, la, b, lb, &ws, &we, &ties, r0, r1);
        out5[0] = 0; out5[1] = la; out5[2] = ws; out5[3] = we; out5[4] = ties;
        const double s2 = P(b, lb, a, la, &ws, &we, &ties, r0, r1);
        if (s2 > sc) { sc = s2; out5[0] = ws; out5[1] = we; out5[2] = 0; out5[3] = lb; out5[4] = ties; *flag = 1; }
    }
    free(r0); free(r1);
    return sc;
}
/* one direction: s (m values, 1 <= m <= n) as the needle; out2 = window start, end */
double partial_c_one(const uint32_t *s, uint32_t m, const uint32_t *t, uint32_t n, uint32_t *out2)
{
    uint32_t *r0 = malloc((n + 1) * 4), *r1 = malloc((n + 1) * 4), ties;
    const double sc = P(s, m, t, n, out2, out2 + 1, &ties, r0, r1);
    free(r0); free(r1);
    return sc;
}
void partial_c_batch(const uint32_t *av, const uint64_t *ao, const uint32_t *bv, const uint64_t *bo, uint64_t rows, double *score,
                     uint32_t *out5, uint32_t *flag)
{
    for (uint64_t r = 0; r < rows; ++r)
        score[r] = partial_c(av + ao[r], (uint32_t)(ao[r + 1] - ao[r]), bv + bo[r], (uint32_t)(bo[r + 1] - bo[r]), out5 + 5 * r, flag + r);
}
"""


def _pack(strings):
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    vals = np.fromiter((ord(c) for s in strings for c in s), dtype=np.uint32, count=int(off[-1]))
    if vals.size == 0:
        vals = np.zeros(1, dtype=np.uint32)
    return off, vals


class CRef:
    """The C brute force, built once per instance into its own temp dir."""

    def __init__(self):
        self._dir = tempfile.TemporaryDirectory(prefix="partial_ref_")
        src = os.path.join(self._dir.name, "partial_ref.c")
        so = os.path.join(self._dir.name, "libpartial_ref.so")
        with open(src, "w") as f:
            f.write(_C_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
        self._L = C.CDLL(so)
        self._L.partial_c_batch.restype = None
        self._L.partial_c_batch.argtypes = [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 3
        self._L.partial_c_one.restype = C.c_double
        self._L.partial_c_one.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]

    def P(self, s: str, t: str):
        """One direction, s the needle (1 <= len(s) <= len(t)) -> (score, window start, window end)."""
        x = np.array([ord(c) for c in s], dtype=np.uint32)
        y = np.array([ord(c) for c in t], dtype=np.uint32)
        out = np.zeros(2, dtype=np.uint32)
        sc = self._L.partial_c_one(x.ctypes.data, len(s), y.ctypes.data, len(t), out.ctypes.data)
        return (float(sc), int(out[0]), int(out[1]))

    def batch(self, A, B):
        """-> (score f64[N], span uint32[N, 4], windows at the maximum uint32[N], second direction won bool[N])."""
        n = len(A)
        ao, av = _pack(A)
        bo, bv = _pack(B)
        score = np.zeros(n, dtype=np.float64)
        out5 = np.zeros((n, 5), dtype=np.uint32)
        flag = np.zeros(n, dtype=np.uint32)
        if n:
            self._L.partial_c_batch(av.ctypes.data, ao.ctypes.data, bv.ctypes.data, bo.ctypes.data, n, score.ctypes.data,
                                    out5.ctypes.data, flag.ctypes.data)
        return score, out5[:, :4].copy(), out5[:, 4].copy(), flag.astype(bool)

    def partial(self, a: str, b: str):
        s, sp, _, _ = self.batch([a], [b])
        return (float(s[0]),) + tuple(int(x) for x in sp[0])


# The issue's known answers: (a, b, score, a span, b span)
KNOWN = [
    ("this is a test", "this is a test!", 1.0, (0, 14), (0, 14)),
    ("abcd", "XXabcdXX", 1.0, (0, 4), (2, 6)),
    ("jonh", "mr john smith", 0.75, (0, 4), (2, 6)),
    ("kitten", "sitting", 0.6666666666666667, (0, 6), (0, 6)),
    ("ab", "ba", 0.6666666666666667, (0, 2), (0, 1)),
    ("aab", "baa", 0.8, (0, 3), (1, 3)),
    ("abcb", "bcbx", 0.8571428571428572, (0, 4), (0, 3)),
    ("müller", "herr mülelr, k.", 0.8333333333333334, (0, 6), (5, 11)),
    ("new york mets", "the wonderful new yorkk mets", 0.9230769230769231, (0, 13), (14, 27)),
    ("abc", "xyz", 0.0, (0, 3), (0, 1)),
    ("", "abc", 0.0, (0, 0), (0, 0)),
    ("", "", 1.0, (0, 0), (0, 0)),
]
