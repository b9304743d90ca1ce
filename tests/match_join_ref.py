"""Reference statement of the match_join contract (strsim_match_join_*): the CPU oracle's score of every (query, candidate) pair
by one of the five reference measures -- best_match_ref.score_matrix's statement, the oracle held to 16 threads -- then the brute
force of join_ref.from_scores: pair (i, j) is a hit iff score >= min_score, and j > i under `upper`; CSR with every row in ascending
candidate index."""
import os

import numpy as np

import join_ref
import oracle_lib as O

MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")
THREADS = min(16, os.cpu_count() or 4)


def score_matrix(measure, queries, candidates):
    """f64 [len(queries), len(candidates)] from the CPU oracle, over explicit pair columns (best_match_ref.score_matrix)."""
    n, m = len(queries), len(candidates)
    if n == 0 or m == 0:
        return np.zeros((n, m), dtype=np.float64)
    A = [q for q in queries for _ in range(m)]
    B = list(candidates) * n
    return O.batch_strings(measure, A, B, THREADS).reshape(n, m)


def join(measure, queries, candidates, min_score=None, upper=False):
    return join_ref.from_scores(score_matrix(measure, list(queries), list(candidates)), min_score, upper)


from_scores = join_ref.from_scores
same = join_ref.same
