"""The frames of the qgram_join GPU tests and their reference results (tests/qgram_join_ref.py), generated once and shared.  Every
parity frame comes with cutoffs at which 0 < nnz < nq * nc on the reference side: tests/test_qgram_join_cpu.py checks that without a
GPU, the GPU tests assert it again before they compare."""
import functools
import random

import numpy as np

import qgram_join_ref as R

KINDS = R.KINDS
LOWER = "abcdefghijklmnopqrstuvwxyz"
MODES = [(q, multiset) for q in (1, 2, 3) for multiset in (True, False)]

# ---- known answers: every string against every string --------------------------------------------------------------------------
KNOWN_STRINGS = ["night", "nacht", "nigh", "abab", "baba", "abc", "cba", "aaaa", "aa", "a", "b", "", "ab", "Night", "a\0", "a\0\0"]
KNOWN_CUT = 0.5


def _edited(rng, s, alphabet, edits):
    s = list(s)
    for _ in range(edits):
        op = rng.randrange(3)
        p = rng.randrange(len(s) + 1)
        if op == 0 and len(s) < 32:
            s.insert(p, rng.choice(alphabet))
        elif op == 1 and len(s) > 1:
            del s[min(p, len(s) - 1)]
        elif s:
            s[min(p, len(s) - 1)] = rng.choice(alphabet)
    return "".join(s)


@functools.lru_cache(maxsize=None)
def near_duplicates(n=300, seed=41):
    """n ASCII strings of 1 .. 32 bytes: near copies (0 .. 2 edits) of 60 stems in random order; row 1 is a copy of row 0, so that
    the corners of one query have a hit beside the diagonal"""
    rng = random.Random(seed)
    stems = ["".join(rng.choice(LOWER[:12]) for _ in range(1 + (7 * k) % 32)) for k in range(60)]
    out = [_edited(rng, rng.choice(stems), LOWER[:12], rng.randint(0, 2)) for _ in range(n)]
    out[1] = out[0]
    assert all(1 <= len(s) <= 32 for s in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def near_matrix(kind, q, multiset):
    """the reference scores of near_duplicates() against itself: computed once, read-only; a sub-frame is a corner of it"""
    X = list(near_duplicates())
    M = R.score_matrix(kind, X, X, q, multiset)
    M.setflags(write=False)
    return M


GEOMETRY_NQ = (1, 63, 64, 65, 256, 257)
GEOMETRY_NC = (1, 64, 65, 300)
GEOMETRY_CUT = 0.8


def geometry(kind, q, multiset, nq, nc):
    """(Q, Cs, scores) of the nq x nc corner"""
    X = near_duplicates()
    return list(X[:nq]), list(X[:nc]), np.ascontiguousarray(near_matrix(kind, q, multiset)[:nq, :nc])


# ---- the boundary frame ----------------------------------------------------------------------------------------------------------
LONG33 = "abcdefghij klmnopqrst uvwxyzabcde"


@functools.lru_cache(maxsize=None)
def boundary(q):
    """(Q, Cs): lengths 0, q - 1, q, q + 1, 31, 32 and 33 on either side (33: the first slow string), equal strings shorter than q,
    NULs, repeated grams, rows of the 5-plane and the 7-plane form, non-ASCII rows of lane-class length"""
    assert len(LONG33) == 33
    stem = LONG33.replace(" ", "x")
    by_len = [stem[:n] for n in sorted({0, q - 1, q, q + 1, 31, 32, 33})]
    Q = by_len + ["a\0", "a\0\0", "aaaa", "aa", "ab", "ba", "Night", "night", "NIGHT 42", "müller", "muller", "日本", LONG33, "a", "b", ""]
    Cs = [s[::-1] if len(s) > 3 and k % 2 else s for k, s in enumerate(by_len)] + \
         ["a\0\0", "a\0", "aa", "aaaa", "ab", "ab", "night", "Night", "night 42", "muller", "müller", "本日", LONG33[:32], LONG33, "a", "", "b"]
    return tuple(Q), tuple(Cs)


BOUNDARY_CUT = 0.5


@functools.lru_cache(maxsize=None)
def boundary_matrix(kind, q, multiset):
    Q, Cs = boundary(q)
    M = R.score_matrix(kind, list(Q), list(Cs), q, multiset)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def known_matrix(kind, q, multiset):
    M = R.score_matrix(kind, KNOWN_STRINGS, KNOWN_STRINGS, q, multiset)
    M.setflags(write=False)
    return M


def not_vacuous(M, cut, upper=False):
    """0 < nnz < the pairs of the frame on the reference side (nq * nc; under upper the pairs with j > i).  A frame of fewer than
    two pairs -- the 1 x 1 corner, or one candidate under upper -- cannot lie strictly between: there the only demand is that the
    reference has an answer, and the tests compare it at a second cutoff with the other outcome."""
    indptr = R.from_scores(M, cut, upper)[0]
    n, m = M.shape
    total = int((np.arange(m)[None, :] > np.arange(n)[:, None]).sum()) if upper else n * m
    return total < 2 or 0 < int(indptr[-1]) < total


# ---- the cluster frame -----------------------------------------------------------------------------------------------------------
CLUSTER_CUT = 0.8


@functools.lru_cache(maxsize=None)
def cluster_column():
    """near duplicates behind a chain a ~ b ~ c whose ends do not match at bigram Dice 0.8"""
    chain = ["abcdefghijkl", "abcdefghijklmn", "cdefghijklmnop"]
    return tuple(chain + list(near_duplicates()[:120]))
