"""Reference statement of the join contract (strsim_join_*): a brute force over the pairwise scores of extract_ref.score_matrix
(indel_ref for "ratio", token_ref's token_sort_ratio for "token_sort_ratio") -- pair (i, j) is a hit iff score >= score_cutoff,
and j > i under `upper` -- returned as CSR with every row in ascending candidate index."""
import numpy as np

import extract_ref

SCORERS = extract_ref.SCORERS
# the name Context.join takes
MEASURE = {"ratio": "indel", "token_sort_ratio": "token_sort_ratio"}


def from_scores(scores, score_cutoff=None, upper=False):
    """f64 [N, M] -> (indptr uint64 [N + 1], index uint32 [nnz], score f64 [nnz])"""
    n, m = scores.shape
    hit = np.ones((n, m), dtype=bool) if score_cutoff is None else scores >= score_cutoff
    if upper:
        hit &= np.arange(m)[None, :] > np.arange(n)[:, None]
    indptr = np.zeros(n + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum(hit.sum(axis=1), dtype=np.uint64)
    i, j = np.nonzero(hit)  # row-major: ascending j inside a row
    return indptr, j.astype(np.uint32), scores[i, j].astype(np.float64)


def join(scorer, queries, candidates, score_cutoff=None, upper=False):
    return from_scores(extract_ref.score_matrix(scorer, list(queries), list(candidates)), score_cutoff, upper)


def same(got, exp):
    """indptr and indices equal, scores bit for bit"""
    (gp, gi, gs), (ep, ei, es) = got, exp
    return (np.array_equal(np.asarray(gp).astype(np.uint64), np.asarray(ep).astype(np.uint64))
            and np.array_equal(np.asarray(gi).astype(np.int64), np.asarray(ei).astype(np.int64))
            and np.array_equal(np.ascontiguousarray(gs, dtype=np.float64).view(np.uint64), np.ascontiguousarray(es, dtype=np.float64).view(np.uint64)))
