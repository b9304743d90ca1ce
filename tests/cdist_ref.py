"""Reference statement of the cdist contract (strsim_cdist_*): the score of every (query, candidate) pair from the models the
searches are tested against -- best_match_ref.score_matrix (the CPU oracle) for the reference measures, extract_ref.score_matrix
(indel_ref / token_ref) for ratio and token_sort_ratio -- and rapidfuzz's cutoff rule: a score below the cutoff is 0.0."""
import numpy as np

import best_match_ref
import extract_ref

MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice", "ratio", "token_sort_ratio")
# the name Context.cdist takes
MEASURE = {m: m for m in MEASURES}
MEASURE["ratio"] = "indel"


def score_matrix(measure, queries, candidates):
    """f64 [len(queries), len(candidates)]"""
    if measure in extract_ref.SCORERS:
        return extract_ref.score_matrix(measure, list(queries), list(candidates))
    return best_match_ref.score_matrix(measure, list(queries), list(candidates))


def apply_cutoff(scores, score_cutoff=None):
    if score_cutoff is None:
        return scores
    return np.where(scores < score_cutoff, 0.0, scores)


def cdist(measure, queries, candidates, score_cutoff=None):
    return apply_cutoff(score_matrix(measure, queries, candidates), score_cutoff)


def same(a, b):
    """bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
