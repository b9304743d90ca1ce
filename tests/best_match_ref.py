"""Reference statement of the best-match contract (strsim_best_match_*): the oracle's score of every (query, candidate) pair, then
a NumPy top-k -- descending score, ties to the lower candidate index, scores below min_score dropped, empty slots (-1, NaN)."""
import os

import numpy as np

import oracle_lib as O


def score_matrix(measure, queries, candidates):
    """f64 [len(queries), len(candidates)] from the CPU oracle, over explicit pair columns."""
    n, m = len(queries), len(candidates)
    if n == 0 or m == 0:
        return np.zeros((n, m), dtype=np.float64)
    A = [q for q in queries for _ in range(m)]
    B = list(candidates) * n
    return O.batch_strings(measure, A, B, os.cpu_count() or 4).reshape(n, m)


def topk(scores, k, min_score=None):
    """scores f64 [n, m] -> (index int64 [n, k] with -1 for empty, score f64 [n, k] with NaN for empty)."""
    n, m = scores.shape
    idx = np.full((n, k), -1, dtype=np.int64)
    val = np.full((n, k), np.nan, dtype=np.float64)
    cols = np.arange(m)
    for i in range(n):
        row = scores[i]
        keep = cols if min_score is None else cols[row >= min_score]
        order = keep[np.lexsort((keep, -row[keep]))][:k]
        idx[i, :order.size] = order
        val[i, :order.size] = row[order]
    return idx, val


def brute_topk(scores, k, min_score=None):
    """The same by a plain sort of (-score, index) tuples: the cross-check of topk()."""
    n, m = scores.shape
    idx = np.full((n, k), -1, dtype=np.int64)
    val = np.full((n, k), np.nan, dtype=np.float64)
    for i in range(n):
        items = sorted((-float(scores[i, j]), j) for j in range(m) if min_score is None or scores[i, j] >= min_score)[:k]
        for s, (neg, j) in enumerate(items):
            idx[i, s] = j
            val[i, s] = -neg
    return idx, val
