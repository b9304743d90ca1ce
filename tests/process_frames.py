"""The frames of the default_process tests (tests/test_process_gpu.py, tests/test_process_plugin_gpu.py).

Every code point used is older than Unicode 6, so the model (tests/process_ref.py) gives the same answers under any Python 3.
"""
import functools
import random

import process_ref as R

LANE_MAX_BYTES = 64  # = PROCESS_LANE_MAX_BYTES (tests/test_process_cpu.py checks it against the header)

ASCII_KEPT = "abcxyzABCXYZ0189_"
ASCII_JUNK = " ,.-!/()'&\t\n\0@[`{~"
GROWERS = "ȺȾ"                                # two bytes of UTF-8 -> three
SHRINKERS = "KİẞΩÅ"            # K, I with dot, capital sharp s, ohm, angstrom
FOUR_BYTE_LETTERS = "\U00010400\U00010427\U00010428"    # Deseret: upper, upper, lower
FOUR_BYTE_OTHER = "\U0001D11E\U0001F000"                # a musical symbol, a mahjong tile: not word characters
OTHER = "ÀÉßéЖжΣσ漢字١²́　 —¿"
POOL = [ASCII_KEPT, ASCII_JUNK, GROWERS, SHRINKERS, FOUR_BYTE_LETTERS, FOUR_BYTE_OTHER, OTHER]


def _ascii_row(rng, n, kind):
    if kind == 0:    # junk at both ends
        lead, trail = rng.randint(0, n // 3), rng.randint(0, n // 3)
        mid = "".join(rng.choice(ASCII_KEPT + ASCII_JUNK) for _ in range(n - lead - trail))
        return "".join(rng.choice(ASCII_JUNK) for _ in range(lead)) + mid + "".join(rng.choice(ASCII_JUNK) for _ in range(trail))
    if kind == 1:    # nothing survives
        return "".join(rng.choice(ASCII_JUNK) for _ in range(n))
    if kind == 2:    # nothing is trimmed
        return "".join(rng.choice(ASCII_KEPT) for _ in range(n))
    if kind == 3:    # one kept byte, anywhere
        at = rng.randrange(n) if n else 0
        return "".join("Q" if i == at else rng.choice(ASCII_JUNK) for i in range(n))
    return "".join(rng.choice(ASCII_KEPT + ASCII_JUNK + "_\0") for _ in range(n))


def _mixed_row(rng, chars):
    weights = [6, 4, 1, 1, 1, 1, 3]
    return "".join(rng.choice(rng.choices(POOL, weights)[0]) for _ in range(chars))


def _to_bytes(rng, target, alphabet):
    """A string over `alphabet` of exactly `target` bytes of UTF-8 (ASCII fills the last bytes)."""
    s, n = [], 0
    while n < target:
        c = rng.choice(alphabet)
        b = len(c.encode("utf-8"))
        if n + b > target:
            c, b = rng.choice("aZ ,"), 1
        s.append(c)
        n += b
    return "".join(s)


@functools.lru_cache(maxsize=None)
def frame():
    """About 3 000 rows: every length around the lane limit, junk at the ends, rows that process to empty, the growers and
    shrinkers, four-byte letters and non-letters, a combining mark and U+3000, rows of 1 025 bytes and one of about 5 000."""
    rng = random.Random(19)
    rows = []
    for n in range(LANE_MAX_BYTES + 2):                         # ASCII: 0 .. limit + 1 bytes, five kinds each
        for kind in range(5):
            rows.append(_ascii_row(rng, n, kind))
    everything = "".join(POOL)
    for n in range(LANE_MAX_BYTES + 2):                         # non-ASCII at the same byte lengths
        rows.append(_to_bytes(rng, n, everything))
    for n in (63, 64, 65, 66, 67, 127, 128, 129, 130, 191, 192, 193):   # scalar values across the wave's 64-byte chunks
        for alphabet in (GROWERS + "a ", FOUR_BYTE_LETTERS + FOUR_BYTE_OTHER + "b,", SHRINKERS + OTHER, everything):
            rows.append(_to_bytes(rng, n, alphabet))
    for _ in range(2100):
        rows.append(_mixed_row(rng, rng.randint(0, 40)))
    for _ in range(400):                                        # names as they come: mixed-case ASCII with punctuation
        rows.append(_ascii_row(rng, rng.randint(0, 32), rng.choice((0, 0, 4))))
    rows += ["", " ", "!!!", "　 —", "\U0001D11E", "́", "_", "\0", "\0a\0", "Apple, Inc.", "apple inc",
             "ÀÉ　x", "é", GROWERS * 40, "Ⱥ", "K"]
    # spaces in front of, between and behind the kept scalar values that span whole chunks
    rows += [" " * 70 + "É" + "," * 70 + "x" + "\t" * 130, "　" * 50 + "A" + "　" * 50, "." * 200 + "é",
             "é" + "." * 200, " " * 64 + "Ж", " " * 63 + "Ж" + " " * 64, "," * 300 + "—"]
    for n in (1025, 1025, 1025):
        rows.append(_to_bytes(rng, n, everything))
    rows.append(_to_bytes(rng, 1025, ASCII_KEPT + ASCII_JUNK))  # ASCII, but beyond the lane tier
    rows.append(_to_bytes(rng, 5003, everything))
    rng.shuffle(rows)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def expected():
    return tuple(R.default_process(s) for s in frame())


def is_lane_row(s):
    """Does the lane tier take the row (ASCII, at most LANE_MAX_BYTES bytes)?"""
    b = s.encode("utf-8")
    return len(b) <= LANE_MAX_BYTES and all(x < 0x80 for x in b)


@functools.lru_cache(maxsize=None)
def pair_frame():
    """(A, B) of 600 rows for processed scoring: names that differ in case, punctuation and a few edits, lane and wave rows."""
    rng = random.Random(23)
    A, B = [], []
    words = ["Apple", "Inc.", "GmbH", "École", "Zürich", "O'Neil", "AT&T", "Жук", "ȺB", "Kelvin", "co-op", "_x_",
             "\U00010400\U00010401", "l’été", "Nº5", "foo_bar", "a", "B2B", "漢字"]
    seps = [" ", ", ", "  ", "-", " & ", ". ", "　", "/"]
    for _ in range(600):
        toks = [rng.choice(words) for _ in range(rng.randint(0, 5))]
        a = "".join(t + rng.choice(seps) for t in toks)
        other = list(toks)
        rng.shuffle(other)
        if other and rng.random() < 0.5:
            other[rng.randrange(len(other))] = rng.choice(words)
        b = rng.choice(["", " ", "!"]) + rng.choice(seps).join(t.swapcase() if rng.random() < 0.5 else t for t in other)
        if rng.random() < 0.05:
            b = b * 12  # beyond the lane tiers
        A.append(a)
        B.append(b)
    return tuple(A), tuple(B)
