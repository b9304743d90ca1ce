"""Reference statement of the extract contract (strsim_extract_*): the score of every (query, candidate) pair from indel_ref
(scorer "ratio") or token_ref's token_sort_ratio (scorer "token_sort_ratio"), then best_match_ref's NumPy top-k -- descending score,
ties to the lower candidate index, scores below score_cutoff dropped, empty slots (-1, NaN)."""
import numpy as np

import best_match_ref
import indel_ref
import token_ref

SCORERS = ("ratio", "token_sort_ratio")


def score_matrix(scorer, queries, candidates):
    """f64 [len(queries), len(candidates)] over explicit pair columns."""
    n, m = len(queries), len(candidates)
    if n == 0 or m == 0:
        return np.zeros((n, m), dtype=np.float64)
    if scorer == "token_sort_ratio":
        # token_ref.token_sort_ratio(a, b) = indel(token_sort(a), token_sort(b)): each string normalised once, then the same
        # Indel score (indel_ref.normalise and token_ref.E are the same two f64 operations)
        queries = [token_ref.token_sort(s) for s in queries]
        candidates = [token_ref.token_sort(s) for s in candidates]
    elif scorer != "ratio":
        raise ValueError(scorer)
    if m >= 10_000:  # (batch_numpy encodes every pair's strings anew: too slow for a few queries against a long column)
        return _few_against_many(queries, candidates)
    A = [q for q in queries for _ in range(m)]
    B = list(candidates) * n
    return indel_ref.batch_numpy(A, B).reshape(n, m)


def _few_against_many(queries, candidates):
    """The same scores for a few queries against a long column: the column encoded once, then indel_ref.batch_numpy_lcs's
    recurrence for one query against every candidate at a time, and indel_ref.scores_from_distances."""
    m = len(candidates)
    lc = np.array([len(s) for s in candidates], dtype=np.int64)
    L = max(int(lc.max(initial=0)), 1)
    Y = np.full((m, L), -2, dtype=np.int32)  # (the pad never matches: cells past a string's end repeat the last real one)
    for r, s in enumerate(candidates):
        if s:
            Y[r, :len(s)] = [ord(ch) for ch in s]
    out = np.empty((len(queries), m), dtype=np.float64)
    for i, q in enumerate(queries):
        prev = np.zeros((m, L + 1), dtype=np.int32)
        for ch in q:
            cur = np.zeros_like(prev)
            hit = Y == ord(ch)
            for j in range(1, L + 1):
                cur[:, j] = np.where(hit[:, j - 1], prev[:, j - 1] + 1, np.maximum(prev[:, j], cur[:, j - 1]))
            prev = cur
        d = len(q) + lc - 2 * prev[:, L].astype(np.int64)
        out[i] = indel_ref.scores_from_distances(d, np.full(m, len(q)), lc)
    return out


def topk(scores, k, score_cutoff=None):
    return best_match_ref.topk(scores, k, score_cutoff)


def brute_topk(scores, k, score_cutoff=None):
    return best_match_ref.brute_topk(scores, k, score_cutoff)


def extract(scorer, queries, candidates, k, score_cutoff=None):
    return topk(score_matrix(scorer, queries, candidates), k, score_cutoff)
