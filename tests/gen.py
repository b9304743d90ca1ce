"""Seeded random string-pair generators for parity tests (pure Python, small sizes)."""
import random

ASCII_LOWER = "abcdefghijklmnopqrstuvwxyz"
MIXED = "abcdefghij" + "ABC" + " -'." + "éèüñ" + "日本語" + "😀𝄞"


def rand_string(rng, alphabet, lo, hi):
    return "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))


def edit(rng, s, alphabet, k):
    s = list(s)
    for _ in range(k):
        op = rng.randint(0, 2)
        if op == 0:
            s.insert(rng.randint(0, len(s)), rng.choice(alphabet))
        elif op == 1 and s:
            del s[rng.randrange(len(s))]
        elif s:
            s[rng.randrange(len(s))] = rng.choice(alphabet)
    return "".join(s)


def pairs(seed, n, alphabet=ASCII_LOWER, lo=0, hi=32, p_edit=0.5, p_same=0.05, max_bytes=None):
    """b is an edited copy of a (p_edit), identical (p_same) or independent -- the BASELINE.md input law."""
    rng = random.Random(seed)
    A, B = [], []
    while len(A) < n:
        a = rand_string(rng, alphabet, lo, hi)
        r = rng.random()
        if r < p_edit:
            b = edit(rng, a, alphabet, rng.randint(1, 3))
        elif r < p_edit + p_same:
            b = a
        else:
            b = rand_string(rng, alphabet, lo, hi)
        if max_bytes is not None and (len(a.encode()) > max_bytes or len(b.encode()) > max_bytes):
            continue
        A.append(a)
        B.append(b)
    return A, B


# One batch of the slow-string fallback of the searches and of cdist is 16 literal calls (MATCH_FALLBACK_CALLS): 37 slow strings are
# two full batches and a partial one, 21 are one full batch and a partial one.  (Batches of fewer than 16 calls need more than 2^20
# rows on a side: not tested.)
SLOW_QUERIES, SLOW_CANDIDATES = 37, 21


def outside_lane_class(s, token_sorted=False):
    """is s outside the lane class (non-ASCII, or longer than 32 bytes), as it is or as token_sort leaves it"""
    if token_sorted:
        s = " ".join(sorted(s.split()))
    b = s.encode()
    return len(b) > 32 or any(x > 127 for x in b)


def slow_strings(seed, n, alphabet="abcde"):
    """n distinct strings outside the lane class of the search and cdist kernels (ASCII, at most 32 bytes), alternately a short
    one with a non-ASCII letter and an ASCII one of 33 .. 40 bytes.  Single inner spaces make tokens, so token_sort leaves both
    kinds outside the class."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        s = list(rand_string(rng, alphabet, 3, 11) if len(out) % 2 == 0 else rand_string(rng, alphabet, 33, 40))
        for i in range(4, len(s) - 1, 6):
            s[i] = " "
        if len(out) % 2 == 0:  # (behind the spaces, at a letter's place: the non-ASCII letter stays)
            s[rng.choice([i for i, ch in enumerate(s) if ch != " "])] = rng.choice("\u00e9\u00f1\u00fc")
        s = "".join(s)
        assert outside_lane_class(s) and outside_lane_class(s, token_sorted=True)
        if s not in out:
            out.append(s)
    return out


def batch_boundary_frame(seed, side, fast=5, alphabet="abcde"):
    """(queries, candidates): `fast` lane-class strings a side and, on the side(s) named ("queries", "candidates", "both"),
    SLOW_QUERIES / SLOW_CANDIDATES slow ones, shuffled."""
    rng = random.Random(seed)
    Q = [rand_string(rng, alphabet + " ", 1, 12).strip() or "a" for _ in range(fast)]
    Cs = [rand_string(rng, alphabet + " ", 1, 12).strip() or "b" for _ in range(fast)]
    if side in ("queries", "both"):
        Q += slow_strings(seed + 1, SLOW_QUERIES, alphabet)
    if side in ("candidates", "both"):
        Cs += slow_strings(seed + 2, SLOW_CANDIDATES, alphabet)
    rng.shuffle(Q)
    rng.shuffle(Cs)
    # the batch shape is pinned, not hoped for: exactly these many slow strings a side, raw and token-sorted
    for X, slow in ((Q, SLOW_QUERIES if side in ("queries", "both") else 0), (Cs, SLOW_CANDIDATES if side in ("candidates", "both") else 0)):
        assert sum(outside_lane_class(s) for s in X) == slow == sum(outside_lane_class(s, token_sorted=True) for s in X)
    return Q, Cs
