"""Transformations of strings that keep a similarity or a distance exactly while they move the pair into another kernel tier, and the
seeded generator of the pairs they are applied to.  Pure Python: plain functions on `str`, no GPU and no library.

Every measure of the library depends only on WHICH characters of a pair are equal (the token measures: also on token boundaries, token
order and nothing else about whitespace), so

  relabel(s, base)       every non-whitespace character c -> chr(ord(c) + base): injective, monotone, no image is whitespace.
                         Equality patterns, token boundaries and the token sort order survive, character counts do not change;
                         bytes per character go from 1 to 2 (0x400), 3 (0x4E00) or 4 (0x1F600).
  affix(p, a, b, s)      (p + a + s, p + b + s): Levenshtein, OSA and Indel distances do not change.
  reverse(s)             both strings reversed: distances, levenshtein / osa / indel / jaccard / sorensen_dice do not change (Jaro's
                         greedy matching and partial_ratio's tie rules are not reversal-invariant).
  shuffle_tokens(...)    one side's tokens permuted and joined again with runs of any whitespace: both token ratios do not change;
                         every token repeated on top of it (copies=): token_set_ratio does not change.

tests/relation_checks.py states the relations over these; tests/test_relations_cpu.py holds the models to them, and
tests/test_relations_gpu.py the kernels.
"""
import random

RELABEL_BASES = (0x400, 0x4E00, 0x1F600)  # images take 2, 3 and 4 bytes of UTF-8
ALPHABETS = ("ab", "abcdef")              # tiny alphabets: ties and long common subsequences
BASE_MAX_LEN = 30                         # a base pair is lane class for every measure (the smallest cap is 32 bytes)

# byte caps a padded pair is placed at (cap: the last length of the lower tier) and one byte past.  Levenshtein: 32 and 128 are the
# similarity's lane tiers; its distance kernel shares OSA's lane cap of 64
AFFIX_CAPS = {"levenshtein": (32, 64, 128, 1024), "osa": (64, 1024), "indel": (128, 1024)}


# ---- transformations ----

def relabel(s, base):
    return "".join(c if c.isspace() else chr(ord(c) + base) for c in s)


def unrelabel(s, base):
    return "".join(c if c.isspace() else chr(ord(c) - base) for c in s)


def reverse(s):
    return s[::-1]


def affix(p, a, b, s=""):
    return p + a + s, p + b + s


def pad_pair_to(rng, a, b, longest, alphabet):
    """(p + a + s, p + b + s) with random p and s over `alphabet` such that the LONGER string has exactly `longest` characters."""
    room = longest - max(len(a), len(b))
    assert room >= 0
    cut = rng.randint(0, room)
    p = "".join(rng.choice(alphabet) for _ in range(cut))
    s = "".join(rng.choice(alphabet) for _ in range(room - cut))
    return affix(p, a, b, s)


def pad_columns_to(seed, A, B, longest, alphabet):
    rng = random.Random(seed)
    out = [pad_pair_to(rng, a, b, longest, alphabet) for a, b in zip(A, B)]
    return [x for x, _ in out], [y for _, y in out]


def shuffle_tokens(rng, s, whitespace, max_run=3, edges=True, copies=1):
    """The tokens of s (each `copies` times) in a random order, joined by runs of 1..max_run characters of `whitespace`, with
    leading and trailing runs of 0..max_run (edges)."""
    toks = s.split() * copies
    rng.shuffle(toks)

    def run(lo):
        return "".join(rng.choice(whitespace) for _ in range(rng.randint(lo, max_run)))

    out = run(0) if edges else ""
    for i, t in enumerate(toks):
        if i:
            out += run(1)
        out += t
    return out + (run(0) if edges else "")


def spread_tokens(rng, s, whitespace, total, max_run=3):
    """shuffle_tokens with `total` more whitespace characters in one gap (leading, between two tokens or trailing, at random): the
    result has more than `total` characters, a string without tokens included."""
    toks = s.split()
    rng.shuffle(toks)
    big = rng.randrange(len(toks) + 1)
    out = ""
    for i in range(len(toks) + 1):
        k = rng.randint(1 if 0 < i < len(toks) else 0, max_run) + (total if i == big else 0)
        out += "".join(rng.choice(whitespace) for _ in range(k))
        if i < len(toks):
            out += toks[i]
    return out


# ---- generator ----

def _rand(rng, alphabet, lo, hi):
    return "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))


def edit(rng, s, alphabet, k):
    """k edits: insert, delete, substitute, swap two adjacent characters."""
    s = list(s)
    for _ in range(k):
        op = rng.randrange(4)
        if op == 0 or not s:
            s.insert(rng.randint(0, len(s)), rng.choice(alphabet))
        elif op == 1:
            del s[rng.randrange(len(s))]
        elif op == 2:
            p = rng.randrange(len(s))
            s[p] = rng.choice([c for c in alphabet if c != s[p]])
        elif len(s) >= 2:
            p = rng.randrange(len(s) - 1)
            s[p], s[p + 1] = s[p + 1], s[p]
    return "".join(s)


def pairs(seed, n, alphabet, lo=0, hi=BASE_MAX_LEN, p_edit=0.6, p_same=0.05, p_empty=0.03):
    """n pairs of at most `hi` characters each: b is a copy of a with 1..3 edits (p_edit), a itself (p_same), one or both sides
    empty (p_empty), or independent."""
    rng = random.Random(seed)
    A, B = [], []
    while len(A) < n:
        a = _rand(rng, alphabet, lo, hi)
        r = rng.random()
        if r < p_edit:
            b = edit(rng, a, alphabet, rng.choice((1, 2, 2, 3)))
        elif r < p_edit + p_same:
            b = a
        elif r < p_edit + p_same + p_empty:
            a, b = rng.choice((("", _rand(rng, alphabet, lo, hi)), (a, ""), ("", "")))
        else:
            b = _rand(rng, alphabet, lo, hi)
        if len(b) > hi:
            continue
        if rng.random() < 0.5:
            a, b = b, a
        A.append(a)
        B.append(b)
    return A, B


def frame(seed, n):
    """Half of the pairs over each alphabet, shuffled."""
    A, B = [], []
    for i, al in enumerate(ALPHABETS):
        x, y = pairs(seed * 16 + i, n // len(ALPHABETS) + (i < n % len(ALPHABETS)), al)
        A += x
        B += y
    idx = list(range(len(A)))
    random.Random(seed).shuffle(idx)
    return [A[i] for i in idx], [B[i] for i in idx]


def token_pairs(seed, n, alphabet, max_len=BASE_MAX_LEN):
    """Pairs of token strings of at most max_len characters: 1..5 tokens of 1..4 letters joined by one space; b holds a's tokens,
    some edited, shuffled, one added or dropped (half of the rows), or is independent; a few rows have no token."""
    rng = random.Random(seed)

    def toks():
        return [_rand(rng, alphabet, 1, 4) for _ in range(rng.randint(1, 5))]

    A, B = [], []
    while len(A) < n:
        ta = toks()
        r = rng.random()
        if r < 0.55:
            tb = [edit(rng, t, alphabet, 1) or "a" if rng.random() < 0.5 else t for t in ta]
            rng.shuffle(tb)
            q = rng.random()
            if q < 0.3:
                tb.append(_rand(rng, alphabet, 1, 4))
            elif q < 0.5 and len(tb) > 1:
                tb.pop()
        elif r < 0.58:
            tb = []
        else:
            tb = toks()
        a, b = " ".join(ta), " ".join(tb)
        if len(a) > max_len or len(b) > max_len:
            continue
        if rng.random() < 0.5:
            a, b = b, a
        A.append(a)
        B.append(b)
    return A, B


def token_frame(seed, n):
    A, B = [], []
    for i, al in enumerate(ALPHABETS):
        x, y = token_pairs(seed * 16 + i, n // len(ALPHABETS) + (i < n % len(ALPHABETS)), al)
        A += x
        B += y
    idx = list(range(len(A)))
    random.Random(seed).shuffle(idx)
    return [A[i] for i in idx], [B[i] for i in idx]


def search_frame(seed, nq, nc, alphabet="abcdef", lo=0, hi=12):
    """Queries and candidates of a search: the candidates random, every query a candidate with 0..3 edits (two thirds) or random."""
    rng = random.Random(seed)
    Cs = [_rand(rng, alphabet, lo, hi) for _ in range(nc)]
    Q = []
    while len(Q) < nq:
        q = edit(rng, rng.choice(Cs), alphabet, rng.randint(0, 3)) if rng.random() < 0.67 else _rand(rng, alphabet, lo, hi)
        if len(q) <= hi:
            Q.append(q)
    return Q, Cs


def token_search_frame(seed, nq, nc, alphabet="abcdef"):
    A, B = token_pairs(seed, max(nq, nc), alphabet, max_len=20)
    return A[:nq], B[:nc]
