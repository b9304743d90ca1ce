"""Reference statement of the qgram_join contract (strsim_qgram_join_*): qgram_ref.batch over every (query, candidate) pair, then the
brute force of join_ref.from_scores: pair (i, j) is a hit iff score >= min_score, and j > i under `upper`; CSR with every row in
ascending candidate index.  Plain Python: the frames of the tests are small."""
import numpy as np

import join_ref
import qgram_ref

KINDS = qgram_ref.KINDS

# The known answers: query, candidate, kind, q, multiset, score
KNOWN = [
    ("night", "nacht", "sorensen_dice", 2, True, 0.25),
    ("night", "nacht", "jaccard", 2, True, 1 / 7),
    ("abab", "baba", "jaccard", 2, True, 0.5),
    ("abab", "baba", "jaccard", 2, False, 1.0),
    ("abc", "cba", "jaccard", 1, True, 1.0),
    ("abc", "cba", "jaccard", 2, True, 0.0),
    ("aaaa", "aa", "jaccard", 2, False, 1.0),
    ("aaaa", "aa", "sorensen_dice", 2, True, 0.5),
    ("aaaa", "aa", "overlap", 2, True, 1.0),
    ("a", "a", "cosine", 2, True, 1.0),
    ("a", "b", "cosine", 2, True, 0.0),
    ("", "", "overlap", 3, False, 1.0),
    ("ab", "abc", "sorensen_dice", 3, True, 0.0),
]


def score_matrix(kind, queries, candidates, q=2, multiset=True):
    """f64 [len(queries), len(candidates)]: qgram_ref.batch with each query as the literal of a call"""
    n, m = len(queries), len(candidates)
    M = np.zeros((n, m), dtype=np.float64)
    for i, s in enumerate(queries):
        if m:
            M[i] = qgram_ref.batch(kind, [s], list(candidates), q, multiset)
    return M


def join(kind, queries, candidates, min_score=None, q=2, multiset=True, upper=False):
    return join_ref.from_scores(score_matrix(kind, list(queries), list(candidates), q, multiset), min_score, upper)


from_scores = join_ref.from_scores
same = join_ref.same
