"""The frames of the distance_join GPU tests and their reference matrices (tests/distance_join_ref.py), generated once and shared,
read-only.  tests/test_distance_join_cpu.py checks without a GPU that none of them is vacuous on the reference side; the GPU tests
assert it again before they compare."""
import functools
import random

import numpy as np

import damerau_ref
import distance_join_ref as R

MEASURES = R.MEASURES
LOWER = "abcdefghijklmnopqrstuvwxyz"
KS = (0, 1, 2, 3, None)  # None: unbounded

# ---- known answers: every string against every string --------------------------------------------------------------------------
KNOWN_STRINGS = ["ca", "abc", "ac", "", "a", "ab", "ba", "abcdef", "badcfe", "a cat", "an abct", "kitten", "sitting", "a\0", "a\0\0", "Abc"]


@functools.lru_cache(maxsize=None)
def known_matrix(measure):
    M = R.matrix(measure, KNOWN_STRINGS, KNOWN_STRINGS)
    M.setflags(write=False)
    return M


# ---- the near-duplicate frame ----------------------------------------------------------------------------------------------------

def _edited(rng, s, alphabet, edits):
    s = list(s)
    for _ in range(edits):
        op = rng.randrange(3)
        p = rng.randrange(len(s) + 1)
        if op == 0 and len(s) < 32:
            s.insert(p, rng.choice(alphabet))
        elif op == 1 and len(s) > 6:
            del s[min(p, len(s) - 1)]
        elif s:
            s[min(p, len(s) - 1)] = rng.choice(alphabet)
    return "".join(s)


@functools.lru_cache(maxsize=None)
def near_duplicates(n=300, seed=43):
    """n ASCII strings of 1 .. 32 bytes in random order.  70 of them have one or two bytes: against each other their distance is at
    most 2 and every other string is at least 6 bytes long, further than any k of the tests, so the first wave of the length order
    has no undecided pair.  The others are copies of 40 stems of 6 .. 32 bytes with 0 .. 2 edits and then swaps of neighbours and
    swaps across an inserted byte (x y -> y z x: the edit the restricted distance counts as 3 and the unrestricted one as 2).  Row 1
    is a copy of row 0, so that the corners of one query have a hit beside the diagonal."""
    rng = random.Random(seed)
    alpha = LOWER[:12]
    short = ["".join(rng.choice(alpha) for _ in range(1 + k % 2)) for k in range(70)]
    stems = ["".join(rng.choice(alpha) for _ in range(6 + (7 * k) % 27)) for k in range(40)]
    out = []
    for _ in range(n - len(short)):
        kind = rng.randrange(6)
        s = _edited(rng, rng.choice(stems), alpha, rng.randint(0, 2) if kind < 2 else rng.randint(0, 1) * (kind & 1))
        if kind == 1:
            s = damerau_ref.swapped(rng, s, rng.randint(1, 2))
        elif kind in (2, 3, 4) and len(s) < 32:
            s = damerau_ref.gapped(rng, s, 1, alpha)
        elif kind == 5 and len(s) < 31:
            s = damerau_ref.swapped(rng, damerau_ref.gapped(rng, s, 1, alpha), 1)
        out.append(s[:32])
    out += short
    rng.shuffle(out)
    out[0] = next(s for s in out if len(s) >= 12)
    out[1] = out[0]
    assert all(1 <= len(s) <= 32 for s in out) and sum(len(s) <= 2 for s in out) >= 64 and not any(2 < len(s) < 6 for s in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def near_matrix(measure):
    """the reference distances of near_duplicates() against itself: computed once, read-only; a sub-frame is a corner of it"""
    X = list(near_duplicates())
    M = R.matrix(measure, X, X)
    M.setflags(write=False)
    return M


GEOMETRY_NQ = (1, 63, 64, 65, 256, 257)
GEOMETRY_NC = (1, 64, 65, 300)


def geometry(measure, nq, nc):
    """(Q, Cs, distances) of the nq x nc corner"""
    X = near_duplicates()
    return list(X[:nq]), list(X[:nc]), np.ascontiguousarray(near_matrix(measure)[:nq, :nc])


def geometry_ks(nq, nc):
    """the cutoffs of a corner: unbounded only up to 65 x 65"""
    return tuple(k for k in KS if k is not None or (nq <= 65 and nc <= 65))


def not_vacuous(M, k, upper=False):
    """0 < nnz < the pairs of the frame on the reference side (nq * nc; under upper the pairs with j > i).  A frame of fewer than
    two pairs -- the 1 x 1 corner, or one candidate under upper -- cannot lie strictly between, and without a cutoff every pair is a
    hit by definition: there the only demand is that the reference has an answer."""
    n, m = M.shape
    total = int((np.arange(m)[None, :] > np.arange(n)[:, None]).sum()) if upper else n * m
    if k is None:
        return int(R.from_distances(M, None, upper)[0][-1]) == total
    return total < 2 or 0 < int(R.from_distances(M, k, upper)[0][-1]) < total


def undecided(O, lens_q, lens_c, k):
    """bool [N, M]: the pairs the Damerau-Levenshtein sweep cannot decide by the OSA distance O at cutoff k: the lengths are within k
    of each other and 3 <= osa <= 2 k"""
    near = np.abs(np.asarray(lens_q)[:, None] - np.asarray(lens_c)[None, :]) <= k
    return near & (O >= 3) & (O <= 2 * k)


def damerau_frame_report(X, k):
    """What makes a frame a test of the Damerau-Levenshtein sweep at cutoff k >= 2: (hit pairs with dl < osa <= 2 k, undecided pairs
    that are no hits, runs of 64 consecutive queries in length order -- the waves of the sweep -- without an undecided pair)"""
    X = list(X)
    O, D = R.matrix("osa", X, X), R.matrix("damerau_levenshtein", X, X)
    lens = np.array([len(s) for s in X])
    U = undecided(O, lens, lens, k)
    order = np.argsort(lens, kind="stable")
    quiet = sum(1 for w in range(0, len(X) - 63, 64) if not U[order[w:w + 64]].any())
    return int(((D <= k) & (D < O) & (O <= 2 * k)).sum()), int((U & (D > k)).sum()), quiet


# ---- the boundary frame ----------------------------------------------------------------------------------------------------------
LONG33 = "abcdefghij klmnopqrst uvwxyzabcde"
_STEM = LONG33.replace(" ", "x")


@functools.lru_cache(maxsize=None)
def boundary():
    """(Q, Cs): lengths 0, 1, 31, 32 and 33 on either side (33: the first slow string); pairs whose lengths differ by k and k + 1 and
    pairs at d = k and k + 1 for k = 0 .. 3 (a stem of 20 bytes cut and edited); rows of the five-plane form (lower case) and of the
    seven-plane form (mixed case, digits, NULs); non-ASCII rows of lane-class length; a 32-byte candidate against 32-byte queries
    that the OSA distance leaves undecided (swaps across a byte)."""
    assert len(LONG33) == 33
    stem = "abcdefghijklmnopqrst"
    by_len = [_STEM[:n] for n in (0, 1, 31, 32, 33)]
    cuts = [stem[:20 - d] for d in range(0, 6)]                       # | lq - lc | = 0 .. 5 against the stem
    subs = [("X" * d + stem[d:]) for d in range(1, 6)]                  # d = 1 .. 5 by substitutions (mixed case: seven planes)
    full = _STEM[:32]
    gapped = [damerau_ref.gapped_at(full[:31], 3, "z"), damerau_ref.gapped_at(damerau_ref.gapped_at(full[:30], 3, "z"), 12, "q"),
              full[1] + full[0] + full[2:29] + full[30] + "Q" + full[29]]
    Q = by_len + [stem] + subs + gapped + ["ca", "abc", "a\0", "a\0\0", "Night 42", "night", "müller", "muller", "日本", LONG33, "a", ""]
    Cs = [s[::-1] if len(s) > 3 and x % 2 else s for x, s in enumerate(by_len)] + cuts + [stem[:10] + stem[11] + stem[10] + stem[12:]] + \
         [full] + ["abc", "ac", "a\0\0", "a\0", "night", "Night 42", "muller", "müller", "本日", LONG33[:32], LONG33, "a", "", "b"]
    assert len(gapped[0]) == 32 and len(gapped[1]) == 32 and len(gapped[2]) == 32
    return tuple(Q), tuple(Cs)


@functools.lru_cache(maxsize=None)
def boundary_matrix(measure):
    Q, Cs = boundary()
    M = R.matrix(measure, list(Q), list(Cs))
    M.setflags(write=False)
    return M


# ---- the cluster frame -----------------------------------------------------------------------------------------------------------
CLUSTER_K = 2


@functools.lru_cache(maxsize=None)
def cluster_column():
    """near duplicates behind a chain a ~ b ~ c whose links are 2 edits and whose ends are 4 apart"""
    chain = ["qrstuvwxyzqrst", "qrstuvwxyzqrAB", "qrstuvwxyCDrAB"]
    return tuple(chain + list(near_duplicates()))
