"""The frames of the WRatio GPU tests (tests/test_wratio_gpu.py, tests/test_wratio_plugin_gpu.py) and their model columns, built
once per process.

main() is one frame of about 7 000 rows that hits every boundary of the five measures (ids 18 .. 26): length ratios at and either
side of 1.5 and of 8, multi-byte rows whose byte ratio and character ratio fall in different classes, shared-token rows, duplicate
tokens, the 29 whitespace code points, rows beyond the token lane class (more than 64 bytes, more than 16 tokens), haystacks of more
than 32 bytes (the partial wave tier), a handful of needles of more than 64 values, non-ASCII rows, empty and whitespace-only rows.
Tests that need fewer rows or one class take rows of it by index, so that the model runs once.
"""
import functools
import random

import numpy as np

import token_ref as T
import wratio_ref as W

RATIOS = ((2, 3), (4, 6), (5, 7), (3, 4), (6, 9), (7, 10), (1, 8), (4, 32), (1, 9), (4, 33), (2, 16), (2, 17), (8, 12), (9, 13))


def _exact(rng, n, alphabet="abc  "):
    """n characters over the alphabet, the first and the last one never a space"""
    s = [rng.choice(alphabet) for _ in range(n)]
    s[0], s[-1] = rng.choice("abc"), rng.choice("abc")
    return "".join(s)


def _build():
    rng = random.Random(26)
    A, B = [], []

    def add(a, b, both=True):
        A.append(a)
        B.append(b)
        if both:
            A.append(b)
            B.append(a)

    # length ratios at and either side of 1.5 and of 8
    for la, lb in RATIOS:
        for _ in range(12):
            add(_exact(rng, la), _exact(rng, lb))
    # bytes and characters in different classes
    add("éé", "abc")              # 2 / 3 characters: far; 4 / 3 bytes would be near
    add("ééé", "abcd")            # 3 / 4 characters: near; 6 / 4 bytes would be far
    add("é", "abcdefgh")          # 1 / 8: far <= 8; 2 / 8 bytes as well
    add("é", "abcdefghi")         # 1 / 9: far > 8; 2 / 9 bytes would be far <= 8
    add("日本", "ab cd")            # 2 / 5 far; 6 / 5 bytes would be near
    add("日本 語", "ab 日本 cd ef")
    add("ab é", "é ab")
    add("ü" * 20, "u" * 29)        # 20 / 29 characters: near, as 40 / 29 bytes
    add("ü" * 20, "u" * 30)        # 20 / 30 characters: far; 40 / 30 bytes would be near
    # near rows, most of them: token edits, shuffles, shared tokens
    GA, GB = T.gen_frame(2026, 1800)
    A += GA
    B += GB
    letters = "abcdefgh"

    def tok(lo=1, hi=6):
        return "".join(rng.choice(letters) for _ in range(rng.randint(lo, hi)))

    def edit(t):
        i, c = rng.randrange(len(t)), rng.choice(letters)
        return (t[:i] + c + t[i + 1:], t[:i] + c + t[i:], (t[:i] + t[i + 1:]) or c)[rng.randrange(3)]

    for _ in range(3300):  # an edited, shuffled copy: near
        ta = [tok(2, 6) for _ in range(rng.randint(2, 4))]
        tb = [edit(t) if rng.random() < 0.4 else t for t in ta]
        rng.shuffle(tb)
        add(" ".join(ta), " ".join(tb), both=False)
    # far rows: the tokens of a inside a longer b (shared tokens) or not
    for i in range(800):
        ta = [tok() for _ in range(rng.randint(1, 2))]
        tb = [tok() for _ in range(rng.randint(3, 9))]
        if i % 3 == 0:
            tb[rng.randrange(len(tb))] = ta[0]                                  # a common token
        elif i % 3 == 1:
            tb.insert(rng.randrange(len(tb)), "".join(ta) + rng.choice(letters))  # a near copy inside a longer token
        add(" ".join(ta), " ".join(tb), both=(i % 2 == 0))
    # duplicate tokens over a vocabulary of three
    for _ in range(250):
        add(" ".join(rng.choice(("ab", "abc", "b")) for _ in range(rng.randint(1, 5))),
            " ".join(rng.choice(("ba", "cab", "abc")) for _ in range(rng.randint(1, 5))), both=False)
    # the 29 whitespace code points
    for cp in T.WHITESPACE:
        w = chr(cp)
        add("x" + w + "y z", "z" + w + w + "x", both=False)
        add(w + "ab" + w, "ab cd ef gh" + w + "ij", both=False)
        add(w, "a" + w + "b", both=False)
    # beyond the token lane class: more than 64 bytes, more than 16 tokens; haystacks of more than 32 bytes
    for _ in range(12):
        long_a = " ".join(tok(3, 8) for _ in range(12))
        ta = long_a.split()
        rng.shuffle(ta)
        add(long_a, " ".join(ta[:-1] + [tok()]))                                # near, > 64 bytes
        add(" ".join(rng.choice("abcd") for _ in range(20)), " ".join(rng.choice("abcd") for _ in range(22)))  # > 16 tokens
        add(" ".join(ta[:2]), long_a)                                           # far, haystack > 32 bytes
        add(tok(4, 6), " ".join(tok(2, 5) for _ in range(14)))                  # far (> 8 for some), no common token as a rule
    # a handful of needles of more than 64 values
    for k in range(3):
        needle = " ".join(tok(2, 7) for _ in range(16))[:70 + k]
        hay = tok(5, 9) + " " + needle[:40] + tok(1, 3) + needle[40:] + " " + " ".join(tok(2, 6) for _ in range(8 + k))
        add(needle.strip(), hay, both=(k == 0))
    # non-ASCII rows
    uni = ("äb", "ö", "üü", "漢字", "漢", "字", "naïve", "café", "ß", "ab")
    for i in range(120):
        ta = [rng.choice(uni) for _ in range(rng.randint(1, 4))]
        tb = [rng.choice(uni) for _ in range(rng.randint(1, 4 if i % 2 else 9))]
        add(" ".join(ta), " ".join(tb), both=False)
    # empty and whitespace-only rows
    for a, b in (("", ""), ("", "abc"), ("", " "), (" ", "\t"), ("  ", "x"), ("　 ", " "), (" x ", "x"), ("   ", "a b c d e f g h i"),
                 (" " * 70, "a"), (" " * 70, " " * 3), ("", "x" * 80)):
        add(a, b)
    return A, B


@functools.lru_cache(maxsize=None)
def frames():
    return W.Frames()


@functools.lru_cache(maxsize=None)
def main():
    """-> (A, B, columns): the frame and wratio_ref.Frames.columns of it."""
    A, B = _build()
    return A, B, frames().columns(A, B)


def take(idx):
    """Rows idx of the main frame -> (A, B, columns)."""
    A, B, cols = main()
    idx = np.asarray(idx, dtype=np.int64)
    return [A[i] for i in idx], [B[i] for i in idx], {k: v[idx] for k, v in cols.items()}


def rows_of_class(*classes):
    """Indices of the main frame's rows in the given wratio classes, in frame order; rows with a string of more than 40 characters
    left out (the sub-frames of the size and call-form tests stay cheap)."""
    A, B, cols = main()
    keep = np.isin(cols["class"], classes) & np.array([len(a) <= 40 and len(b) <= 40 for a, b in zip(A, B)])
    return np.flatnonzero(keep)


def mixed(n, seed=7):
    """n rows of the main frame of every class, in a fixed random order."""
    idx = rows_of_class(W.EMPTY, W.NEAR, W.FAR8, W.FAR)
    return np.random.default_rng(seed).permutation(idx)[:n]
