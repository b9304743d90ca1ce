"""Independent reference for the Hamming, prefix, postfix and LCSseq calls (strsim_common_* of include/strsim_amd.h).

Plain Python over `str`, hence over Unicode scalar values.  Each kind is a count c(a, b) of what the two strings share:
  hamming  positions i < min(|a|, |b|) with a[i] == b[i] (zip)
  prefix   length of the longest common prefix (a loop)
  postfix  length of the longest common suffix (the prefix of the reversed strings)
  lcs_seq  length of the longest common subsequence (the textbook row DP)
and, as in rapidfuzz.distance.{Hamming, Prefix, Postfix, LCSseq}:  similarity = c,  distance = max(|a|, |b|) - c (for Hamming:
mismatches plus the difference of the lengths, pad=True),  normalised = 1.0 when both are empty, else 1.0 - (d / max(|a|, |b|)) with
exactly these two f64 operations.  With a cutoff k the distance call writes d when d <= k and k + 1 otherwise.

lcs_bits() is Hyyro's bit-parallel LCS on Python integers, for the long rows of the GPU suite where the row DP would take minutes;
tests/test_common_cpu.py holds it, the row DP and tests/indel_ref.py to each other.
"""
import random

import numpy as np

KINDS = ("hamming", "prefix", "postfix", "lcs_seq")
UNBOUNDED = 0xFFFFFFFF
LOWER = "abcdefghijklmnopqrstuvwxyz"


def hamming(a: str, b: str) -> int:
    return sum(x == y for x, y in zip(a, b))


def prefix(a: str, b: str) -> int:
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def postfix(a: str, b: str) -> int:
    return prefix(a[::-1], b[::-1])


def lcs_seq(a: str, b: str) -> int:
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0  # D[i-1][j-1]
        for j, y in enumerate(b, 1):
            up = row[j]
            row[j] = diag + 1 if x == y else max(up, row[j - 1])
            diag = up
    return row[len(b)]


def lcs_bits(a: str, b: str) -> int:
    """the same number: V = (V + (V & Eq)) | (V & ~Eq) per character of b over the rows of a, l = the zero bits of V"""
    eq = {}
    for i, x in enumerate(a):
        eq[x] = eq.get(x, 0) | (1 << i)
    full = (1 << len(a)) - 1
    v = full
    for y in b:
        e = eq.get(y, 0)
        v = ((v + (v & e)) | (v & ~e)) & full
    return len(a) - bin(v).count("1")


_COUNT = {"hamming": hamming, "prefix": prefix, "postfix": postfix, "lcs_seq": lcs_seq}


def count(kind: str, a: str, b: str) -> int:
    if kind == "lcs_seq" and max(len(a), len(b)) > 64:
        return lcs_bits(a, b)
    return _COUNT[kind](a, b)


def distance(kind: str, a: str, b: str) -> int:
    return max(len(a), len(b)) - count(kind, a, b)


def normalise(d: int, la: int, lb: int) -> float:
    if la == 0 and lb == 0:
        return 1.0
    return 1.0 - (float(d) / float(max(la, lb)))


def score(kind: str, a: str, b: str) -> float:
    return normalise(distance(kind, a, b), len(a), len(b))


def clamp(d, k):
    """The distance call's output for cutoff k (None / UNBOUNDED: none): d when d <= k, else k + 1; ints or arrays."""
    if k is None or k == UNBOUNDED:
        return d
    return np.where(np.asarray(d) <= k, d, k + 1).astype(np.uint32) if isinstance(d, np.ndarray) else (d if d <= k else k + 1)


def _broadcast(A, B):
    n = max(len(A), len(B)) if len(A) and len(B) else 0
    return (A * n if len(A) == 1 else A), (B * n if len(B) == 1 else B)


def counts(kind, A, B):
    A, B = _broadcast(list(A), list(B))
    return np.array([count(kind, a, b) for a, b in zip(A, B)], dtype=np.uint32)


def frame(kind, A, B):
    """(counts u32, distances u32, scores f64) of two columns (one of them may be a literal of one row)"""
    A, B = _broadcast(list(A), list(B))
    c = np.array([count(kind, a, b) for a, b in zip(A, B)], dtype=np.uint32)
    m = np.array([max(len(a), len(b)) for a, b in zip(A, B)], dtype=np.uint32)
    d = (m - c).astype(np.uint32)
    s = np.array([normalise(int(x), len(a), len(b)) for x, a, b in zip(d, A, B)], dtype=np.float64)
    return c, d, s


# (kind, a, b, count): the answers the issue pins; the UTF-8 rows share bytes but no character
KNOWN = [
    ("hamming", "karolin", "kathrin", 4), ("hamming", "abc", "abcdef", 3), ("hamming", "éa", "ea", 1),
    ("lcs_seq", "AGGTAB", "GXTXAYB", 4),
    ("prefix", "prefix", "preface", 4), ("postfix", "testing", "running", 3),
    ("prefix", "é", "è", 0), ("prefix", "€", "₭", 0), ("postfix", "é", "©", 0), ("postfix", "€", "Ⴌ", 0),
]
# (kind, a, b, distance)
KNOWN_DISTANCES = [("hamming", "karolin", "kathrin", 3), ("hamming", "abc", "abcdef", 3), ("hamming", "éa", "ea", 1),
                   ("lcs_seq", "AGGTAB", "GXTXAYB", 3)]


# ---- frames of the suites ----

def edited(rng, s, alphabet, k):
    """s with k substitutions, and sometimes a character put in or taken out (which moves everything behind it)"""
    s = list(s)
    for _ in range(k):
        if s:
            s[rng.randrange(len(s))] = rng.choice(alphabet)
    r = rng.random()
    if r < 0.15:
        s.insert(rng.randint(0, len(s)), rng.choice(alphabet))
    elif r < 0.30 and s:
        del s[rng.randrange(len(s))]
    return "".join(s)


def lane_frame(rng, n, hi, alphabet=LOWER):
    """n pairs of U{0..hi} characters: an edited copy (half), a copy with another head or tail (a quarter), the same, or independent"""
    A, B = [], []
    for r in range(n):
        a = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, hi)))
        x = r % 8
        if x < 4:
            b = edited(rng, a, alphabet, rng.randint(0, 3))[:hi]
        elif x == 4:
            cut = rng.randint(0, len(a))
            b = ("".join(rng.choice(alphabet) for _ in range(rng.randint(0, hi - (len(a) - cut)))) + a[cut:])
        elif x == 5:
            cut = rng.randint(0, len(a))
            b = (a[:cut] + "".join(rng.choice(alphabet) for _ in range(rng.randint(0, hi - cut))))
        elif x == 6:
            b = a
        else:
            b = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, hi)))
        A.append(a)
        B.append(b)
    return A, B
