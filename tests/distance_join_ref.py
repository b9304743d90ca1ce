"""Reference statement of the distance_join contract (strsim_distance_join_*): the integer edit distance of every (query, candidate)
pair, then a brute force: pair (i, j) is a hit iff d <= max_distance (None: every pair), and j > i under `upper`; CSR with every row
in ascending candidate index.

Levenshtein and OSA are the plain row-by-row DPs over Unicode scalar values, vectorised over the pairs with numpy (one DP cell of
every pair per step).  The unrestricted Damerau-Levenshtein distance is damerau_ref's full-matrix DP: damerau_ref.distance, and for
the larger frames damerau_ref.CRef, the same DP in C that tests/test_damerau_cpu.py holds to it; a matrix computes every distinct
unordered pair once (d is symmetric by all three measures)."""
import functools

import numpy as np

import damerau_ref

MEASURES = ("levenshtein", "osa", "damerau_levenshtein")

# The known answers: a, b, then d by the three measures
KNOWN = [
    ("ca", "abc", 3, 3, 2),
    ("ca", "ac", 2, 1, 1),
    ("", "", 0, 0, 0),
    ("", "abc", 3, 3, 3),
    ("ab", "", 2, 2, 2),
    ("abc", "abc", 0, 0, 0),
    ("kitten", "sitting", 3, 3, 3),
    ("abcdef", "badcfe", 4, 3, 3),
    ("a cat", "an abct", 4, 4, 3),
    ("müller", "mueller", 2, 2, 2),
]


def _codes(strings):
    """(int64 [n, L] of scalar values padded with -1, which no scalar value is, int64 [n] of lengths)"""
    n = len(strings)
    lens = np.array([len(s) for s in strings], dtype=np.int64)
    L = int(lens.max()) if n else 0
    out = np.empty((n, L), dtype=np.int64)
    out[:] = -1
    for r, s in enumerate(strings):
        out[r, :len(s)] = [ord(c) for c in s]
    return out, lens


def pairs(measure, A, B):
    """int64 [len(A)] of d(A[r], B[r]) by "levenshtein" or "osa": the DP of every pair side by side"""
    assert measure in ("levenshtein", "osa") and len(A) == len(B)
    n = len(A)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    a, la = _codes(A)
    b, lb = _codes(B)
    b = np.where(b < 0, -2, b)  # (the two paddings differ)
    La, Lb = a.shape[1], b.shape[1]
    # row i of D for every pair; a pair's answer is taken from its own last row, rows beyond it are computed and never read
    prev2 = None
    prev = np.tile(np.arange(Lb + 1, dtype=np.int64), (n, 1))
    every = np.arange(n)
    res = lb.copy()  # (row 0: the pairs whose first string is empty)
    for i in range(1, La + 1):
        cur = np.empty((n, Lb + 1), dtype=np.int64)
        cur[:, 0] = i
        ai = a[:, i - 1]
        for j in range(1, Lb + 1):
            v = np.minimum(np.minimum(prev[:, j - 1] + (ai != b[:, j - 1]), prev[:, j] + 1), cur[:, j - 1] + 1)
            if measure == "osa" and i > 1 and j > 1:
                swap = (ai == b[:, j - 2]) & (a[:, i - 2] == b[:, j - 1])
                v = np.where(swap, np.minimum(v, prev2[:, j - 2] + 1), v)
            cur[:, j] = v
        prev2, prev = prev, cur
        done = la == i  # the pairs whose last row this is
        res[done] = cur[every[done], lb[done]]
    return res


@functools.lru_cache(maxsize=1)
def _cref():
    return damerau_ref.CRef()


def matrix(measure, queries, candidates):
    """int64 [len(queries), len(candidates)] of the distances"""
    assert measure in MEASURES
    Q, Cs = list(queries), list(candidates)
    uniq = sorted(set(Q) | set(Cs))
    at = {s: x for x, s in enumerate(uniq)}
    need = sorted({(min(at[q], at[c]), max(at[q], at[c])) for q in set(Q) for c in set(Cs)})
    table = {}
    if measure == "damerau_levenshtein":
        f = damerau_ref.distance if len(need) <= 2000 else _cref().distance
        for x, y in need:
            table[(x, y)] = f(uniq[x], uniq[y])
    elif need:
        d = pairs(measure, [uniq[x] for x, _ in need], [uniq[y] for _, y in need])
        table = dict(zip(need, d.tolist()))
    M = np.zeros((len(Q), len(Cs)), dtype=np.int64)
    for i, q in enumerate(Q):
        for j, c in enumerate(Cs):
            M[i, j] = table[(min(at[q], at[c]), max(at[q], at[c]))]
    return M


def from_distances(M, max_distance=None, upper=False):
    """int [N, M] -> (indptr uint64 [N + 1], index uint32 [nnz], distance uint32 [nnz])"""
    M = np.asarray(M)
    n, m = M.shape
    hit = np.ones((n, m), dtype=bool) if max_distance is None else M <= max_distance
    if upper:
        hit &= np.arange(m)[None, :] > np.arange(n)[:, None]
    indptr = np.zeros(n + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum(hit.sum(axis=1), dtype=np.uint64)
    i, j = np.nonzero(hit)  # row-major: ascending j inside a row
    return indptr, j.astype(np.uint32), M[i, j].astype(np.uint32)


def join(measure, queries, candidates, max_distance=None, upper=False):
    return from_distances(matrix(measure, queries, candidates), max_distance, upper)


def same(got, exp):
    """indptr, indices and distances equal"""
    (gp, gi, gd), (ep, ei, ed) = got, exp
    return (np.array_equal(np.asarray(gp).astype(np.uint64), np.asarray(ep).astype(np.uint64))
            and np.array_equal(np.asarray(gi).astype(np.int64), np.asarray(ei).astype(np.int64))
            and np.array_equal(np.asarray(gd).astype(np.int64), np.asarray(ed).astype(np.int64)))
