"""The model of q-gram similarity: Jaccard, Sorensen-Dice, overlap and cosine over the contiguous q-tuples of code points of two
strings, as multisets (collections.Counter) or as sets.  Plain Python, the yardstick of the q-gram tests."""
import math
from collections import Counter

KINDS = ("jaccard", "sorensen_dice", "overlap", "cosine")

# The known answers: pair, q, multiset, (I, na, nb) or None, {kind: score}
KNOWN = [
    ("night", "nacht", 2, True, (1, 4, 4), {"jaccard": 1 / 7, "sorensen_dice": 0.25, "overlap": 0.25, "cosine": 0.25}),
    ("abab", "baba", 2, True, (2, 3, 3), {"jaccard": 0.5, "sorensen_dice": 2 / 3, "overlap": 2 / 3, "cosine": 2 / 3}),
    ("abab", "baba", 2, False, (2, 2, 2), {"jaccard": 1.0, "sorensen_dice": 1.0, "overlap": 1.0, "cosine": 1.0}),
    ("abc", "cba", 1, True, None, {"jaccard": 1.0}),
    ("abc", "cba", 2, True, None, {"jaccard": 0.0}),
]
# ... and with any of the four kinds: a, b, q, score
KNOWN_ANY = [("a", "a", 2, 1.0), ("a", "b", 2, 0.0), ("", "", 2, 1.0), ("ab", "abc", 3, 0.0)]



def _code_points(s):
    """str (or UTF-8 bytes) -> tuple of code points"""
    if isinstance(s, bytes):
        s = s.decode("utf-8")
    return tuple(ord(c) for c in s)


def grams(s, q):
    """The max(len(s) - q + 1, 0) contiguous q-tuples of the code points of s, in order."""
    v = _code_points(s)
    return [v[i:i + q] for i in range(len(v) - q + 1)]


def counts(a, b, q, multiset=True):
    """-> (I, na, nb)"""
    ga, gb = grams(a, q), grams(b, q)
    if multiset:
        ca, cb = Counter(ga), Counter(gb)
        return sum(min(n, cb[g]) for g, n in ca.items()), len(ga), len(gb)
    sa, sb = set(ga), set(gb)
    return len(sa & sb), len(sa), len(sb)


def score(kind, a, b, q=2, multiset=True):
    """One pair -> float.  a == b is 1.0, then a side without a gram is 0.0, then the formula of `kind`."""
    assert kind in KINDS and q in (1, 2, 3)
    if a == b:
        return 1.0
    i, na, nb = counts(a, b, q, multiset)
    if na == 0 or nb == 0:
        return 0.0
    if kind == "jaccard":
        return i / (na + nb - i)
    if kind == "sorensen_dice":
        return (2.0 * i) / (na + nb)
    if kind == "overlap":
        return float(i) / float(min(na, nb))
    return float(i) / math.sqrt(float(na * nb))


def batch(kind, A, B, q=2, multiset=True):
    """Two lists (either may hold one string: a literal) -> list of floats."""
    n = len(B) if len(A) == 1 else len(A)
    return [score(kind, A[0] if len(A) == 1 else A[r], B[0] if len(B) == 1 else B[r], q, multiset) for r in range(n)]
