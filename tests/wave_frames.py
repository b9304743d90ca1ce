"""The frame of the wave-kernel route tests: one small frame, built once, whose every row is left to k_wave_pairs<M>, grouped by
the route the row takes inside that kernel.

Every pair has a string of more than 128 bytes, so no kernel in front of the wave kernel finishes any of its rows.  Inside the wave
kernel the four measures other than Levenshtein run every row the same way; Levenshtein sorts its rows into BYTES batches (both
strings ASCII, a lane per 64 bytes of the shorter string), SYMBOLS batches (anything else inside the Basic Multilingual Plane, a
lane per 32 scalar values of the shorter string), the anti-diagonal fallback (a scalar value beyond the BMP), the early return of an
empty side, and the rows it leaves to k_huge_pairs (a string of more than 1 024 bytes, unless both have at most 1 024 scalar
values).  The classes below put rows at every one of these and at the sizes where the lane counts change.

"ASCII, m against n": m is the length of the shorter string (the pattern: 1 .. 1 024 bytes), n that of the longer one (129 .. 1 024
bytes).

deal() restates, for a chunk of ASCII rows, how Levenshtein ranks a pool and deals it first-fit into BYTES batches (k_wave_pairs in
strsim_kernel_wave.h: the pool ranking, the first-fit test in front of a row, the flushes around the BYTES staging); it shares no
code with the kernel, and nothing on the device reports a flush or a skip: the device test compares results only.
"""
import functools
import random
from collections import namedtuple

import oracle_lib as O

CHUNK = 64
WAVE_CAP = 1024     # bytes (the other measures) / scalar values (Levenshtein) per string in k_wave_pairs
LEV_JOBS = 16       # pairs per batch, at most
ARENA0_BYTES = 8192
TXT_PAD = 48
PATTERN_SIZES = [1, 63, 64, 65, 128, 129, 1024]  # ASCII: the lane count of a job changes behind 64, 128, ...
SYMBOL_SIZES = [31, 32, 33, 64, 65]               # non-ASCII: ... behind 32, 64

ASCII_LOWER = "abcdefghijklmnopqrstuvwxyz"                                   # bits 5 and 6 constant: five planes
ASCII_MIXED = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ .,;-'!?"   # seven planes
CYRILLIC = "".join(chr(c) for c in range(0x0430, 0x0450))                    # one block: the scalar values differ below bit 7
LATIN_CYRILLIC = "abcdefgh" + CYRILLIC[:16]                                  # ... below bit 11
MIXED = "abcxyz" + CYRILLIC[:6] + "語漢字日本中文"                              # Latin + Cyrillic + CJK: up to bit 14
CJK = "".join(chr(c) for c in range(0x4E00, 0x9FA6, 0x0355))                 # bits 11 and up differ inside the alphabet
ALPHABETS = {"cyrillic": CYRILLIC, "latin_cyrillic": LATIN_CYRILLIC, "mixed": MIXED, "cjk": CJK}
ASTRAL = "😀𝄞"

LITERALS = {"ascii": ("the quick brown fox jumps over the lazy dog; " * 5)[:200],  # 200 bytes
            "cyrillic": CYRILLIC[:25] * 4}                                         # 100 letters

Frame = namedtuple("Frame", "A B classes")  # A, B: tuples of str; classes: {name: range of rows}


def _rand(rng, alphabet, n):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _pattern_of(rng, text, alphabet, m):
    """m characters that resemble a slice of text: a copy with about one character in eight replaced"""
    at = rng.randint(0, len(text) - m) if m <= len(text) else 0
    s = list(text[at:at + m])
    s += [rng.choice(alphabet) for _ in range(m - len(s))]
    for i in range(len(s)):
        if rng.random() < 0.125:
            s[i] = rng.choice(alphabet)
    return "".join(s)


def _pair(rng, alphabet, m, n, pattern_in_a):
    text = _rand(rng, alphabet, n)
    pat = _pattern_of(rng, text, alphabet, m)
    return (pat, text) if pattern_in_a else (text, pat)


def _first_chunk(rng):
    """64 ASCII rows for one pool of Levenshtein: six rows of 1 024 against 1 024 bytes (16 lanes each: four fill a batch), four of
    800 against 1 000 (13 lanes: behind 16 + 3 x 13 lanes the fourth does not fit and is skipped), and 54 one-lane rows, which run
    into the limit of 16 jobs per batch"""
    rows = [_pair(rng, ASCII_LOWER, 1024, 1024, i % 2 == 0) for i in range(6)]
    rows += [_pair(rng, ASCII_LOWER, 800, 1000, i % 2 == 0) for i in range(4)]
    rows += [_pair(rng, ASCII_MIXED if i % 3 == 0 else ASCII_LOWER, rng.randint(1, 64), rng.randint(129, 400), i % 2 == 0) for i in range(54)]
    rng.shuffle(rows)
    return rows


def _build():
    rng = random.Random(20260)
    groups = [("one_pool", _first_chunk(rng))]
    for name, alphabet in (("ascii_lower", ASCII_LOWER), ("ascii_mixed", ASCII_MIXED)):
        groups.append((name, [_pair(rng, alphabet, m, max(m, rng.randint(129, 1024)), side) for m in PATTERN_SIZES for side in (True, False)]))
    # an ASCII string against a non-ASCII one: the ASCII staging refuses the pair, it joins a SYMBOLS batch
    groups.append(("ascii_vs_non_ascii", [(_rand(rng, ASCII_LOWER, 200), _rand(rng, CYRILLIC, 90)), (_rand(rng, CYRILLIC, 40), _rand(rng, ASCII_MIXED, 300)),
                                         (_rand(rng, ASCII_LOWER, 150)[:-1] + "é", _rand(rng, ASCII_LOWER, 140)),
                                         (_rand(rng, ASCII_LOWER, 1000), _rand(rng, ASCII_LOWER, 30) + "я")]))
    for name, alphabet in ALPHABETS.items():
        groups.append(("symbols_" + name, [_pair(rng, alphabet, m, rng.randint(130, 300), side) for m in SYMBOL_SIZES for side in (True, False)]))
    # a scalar value beyond the BMP in a string of more than 32 values: the anti-diagonal fallback
    groups.append(("beyond_bmp", [(_rand(rng, ASCII_LOWER, 40) + ASTRAL[0] + _rand(rng, ASCII_LOWER, 100), _rand(rng, ASCII_LOWER, 150)),
                                 (_rand(rng, CYRILLIC, 100), _rand(rng, CYRILLIC + ASTRAL, 80) + ASTRAL[1]),
                                 (_rand(rng, ASTRAL, 50), _rand(rng, ASTRAL, 33)),
                                 (_rand(rng, MIXED, 200), ASTRAL[0] + _rand(rng, MIXED, 33))]))
    groups.append(("empty_side", [("", _rand(rng, ASCII_LOWER, 129)), (_rand(rng, ASCII_MIXED, 700), ""), ("", _rand(rng, CYRILLIC, 70)),
                                 (_rand(rng, CJK, 300), "")]))
    # more than 1 024 bytes, at most 1 024 scalar values: Levenshtein keeps the row (SYMBOLS), the other measures leave it
    long_cyr = _rand(rng, CYRILLIC, 600)
    groups.append(("symbol_route", [(long_cyr, _pattern_of(rng, long_cyr, CYRILLIC, 590)), (_rand(rng, CYRILLIC, 20), _rand(rng, CYRILLIC, 1024)),
                                   (_rand(rng, CJK, 342), _rand(rng, CJK, 100)), (_rand(rng, ASCII_LOWER, 500), _rand(rng, LATIN_CYRILLIC, 900) + "я" * 100)]))
    # more than 1 024 scalar values on one side: every measure leaves the row to k_huge_pairs
    groups.append(("beyond_the_cap", [_pair(rng, ASCII_LOWER, 200, 1025, True), _pair(rng, ASCII_MIXED, 1100, 1300, False),
                                     (_rand(rng, CYRILLIC, 1025), _rand(rng, CYRILLIC, 50)), ("", _rand(rng, ASCII_LOWER, 1030))]))
    A, B, classes = [], [], {}
    for name, rows in groups:
        classes[name] = range(len(A), len(A) + len(rows))
        A += [r[0] for r in rows]
        B += [r[1] for r in rows]
    return Frame(tuple(A), tuple(B), classes)


@functools.lru_cache(maxsize=None)
def frame():
    """the frame; built once, never changed"""
    return _build()


def sides(literal_side=None, literal=None):
    """(A, B) of a call: the frame's columns, or one of them against a one-row side (literal_side 'a': the literal is side a and the
    column is the frame's B)"""
    f = frame()
    if literal_side is None:
        return f.A, f.B
    return ((LITERALS[literal],), f.B) if literal_side == "a" else (f.A, (LITERALS[literal],))


@functools.lru_cache(maxsize=None)
def expected(measure, literal_side=None, literal=None):
    """the oracle's column for that call (cached; read-only)"""
    A, B = sides(literal_side, literal)
    exp = O.batch_strings(measure, list(A), list(B), 8)
    exp.setflags(write=False)
    return exp


# ---- what the classes are made of, from the strings alone ----------------------------------------------------------------------------
def nbytes(s):
    return len(s.encode("utf-8"))


def in_bmp(s):
    return all(ord(c) <= 0xFFFF for c in s)


def vary(a, b):
    """the bits in which the scalar values of the pair differ somewhere"""
    cps = [ord(c) for c in a + b]
    o, n = 0, 0xFFFFFFFF
    for c in cps:
        o |= c
        n &= c
    return o ^ n


def deal(rows):
    """Levenshtein's BYTES batches of one pool of ASCII rows [(a, b)], every string of 1 .. 1 024 bytes: -> (batches, skips, why), the
    batches as lists of row indices in the order they run, the number of times a ranked row was passed over because its lanes did
    not fit, and why each batch was flushed ('lanes', 'jobs', 'arena', 'pass': the end of a pass over the ranking)."""
    assert len(rows) <= 6 * CHUNK and all(a.isascii() and b.isascii() and 1 <= len(a) <= WAVE_CAP and 1 <= len(b) <= WAVE_CAP for a, b in rows)
    m = [min(len(a), len(b)) for a, b in rows]
    n = [max(len(a), len(b)) for a, b in rows]
    order = sorted(range(len(rows)), key=lambda i: (-(n[i] + (m[i] + 31) // 32), i))
    todo, batches, why, skips = list(order), [], [], 0
    cur, lanes, used = [], 0, 0

    def flush(reason):
        nonlocal cur, lanes, used
        if cur:
            batches.append(cur)
            why.append(reason)
        cur, lanes, used = [], 0, 0
    while todo:
        left = []
        for i in todo:
            need = ((m[i] + 31) // 32 + 1) // 2
            if lanes + need > 64:
                skips += 1
                left.append(i)
                continue
            slot = (2 * TXT_PAD + n[i] + 3) & ~3
            if used + slot > ARENA0_BYTES:
                flush("arena")
            cur.append(i)
            lanes += (m[i] + 63) // 64
            used += slot
            if len(cur) == LEV_JOBS:
                flush("jobs")
            elif lanes == 64:
                flush("lanes")
        todo = left
        if todo:
            flush("pass")
    flush("pass")
    return batches, skips, why
