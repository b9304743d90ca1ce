"""Reference statement of the nearest-match contract (strsim_nearest_*): the edit distance of every (query, candidate) pair from
distance_ref, then a NumPy top-k -- ascending distance, ties to the lower candidate index, distances above max_distance dropped,
empty slots (-1, -1)."""
import numpy as np

import distance_ref as D

UNBOUNDED = D.UNBOUNDED
_cdist = None


def distance_matrix(measure, queries, candidates):
    """int64 [len(queries), len(candidates)]: the unbounded distance of every pair (distance_ref.batch_numpy)."""
    n, m = len(queries), len(candidates)
    if n == 0 or m == 0:
        return np.zeros((n, m), dtype=np.int64)
    if m >= 10_000:  # (distance_ref's C DP pair by pair: batch_numpy's code arrays would be pairs x longest string)
        global _cdist
        _cdist = _cdist or D.CDist()
        f, tr = _cdist._L.dist_c, 1 if measure == "osa" else 0
        ys = [(np.array([ord(c) for c in s] or [0], dtype=np.uint32), len(s)) for s in candidates]
        out = np.zeros((n, m), dtype=np.int64)
        for i, q in enumerate(queries):
            x = np.array([ord(c) for c in q] or [0], dtype=np.uint32)
            out[i] = [f(x.ctypes.data, len(q), y.ctypes.data, ly, tr, max(len(q), ly)) for y, ly in ys]
        return out
    A = [q for q in queries for _ in range(m)]
    B = list(candidates) * n
    return D.batch_numpy(measure, A, B).astype(np.int64).reshape(n, m)


def topk(dist, k, max_distance=None):
    """dist int [n, m] -> (index int64 [n, k], distance int64 [n, k]), -1 in both for an empty slot."""
    n, m = dist.shape
    idx = np.full((n, k), -1, dtype=np.int64)
    val = np.full((n, k), -1, dtype=np.int64)
    cols = np.arange(m)
    for i in range(n):
        row = dist[i]
        keep = cols if max_distance is None or max_distance == UNBOUNDED else cols[row <= max_distance]
        order = keep[np.lexsort((keep, row[keep]))][:k]
        idx[i, :order.size] = order
        val[i, :order.size] = row[order]
    return idx, val


def brute_topk(dist, k, max_distance=None):
    """The same by a plain sort of (distance, index) tuples: the cross-check of topk()."""
    n, m = dist.shape
    idx = np.full((n, k), -1, dtype=np.int64)
    val = np.full((n, k), -1, dtype=np.int64)
    for i in range(n):
        items = sorted((int(dist[i, j]), j) for j in range(m)
                       if max_distance is None or max_distance == UNBOUNDED or dist[i, j] <= max_distance)[:k]
        for s, (d, j) in enumerate(items):
            idx[i, s] = j
            val[i, s] = d
    return idx, val
