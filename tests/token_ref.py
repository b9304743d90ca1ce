"""Independent model of token_sort_ratio and token_set_ratio (measure ids 14 and 16): rapidfuzz's fuzz.token_sort_ratio / 100 and
fuzz.token_set_ratio / 100.

Whitespace is Python's str.isspace set (WHITESPACE below, 29 code points), tokens are str.split(), token order is Python's order of
str (lexicographic by scalar value, a proper prefix first), join puts one U+0020 between tokens.  E(d, s) is the library's Indel
epilogue: 1.0 when s == 0, else 1.0 - (d / s), these two f64 operations.

  token_sort(s)            join(sorted(tokens(s)))
  token_sort_ratio(a, b)   indel(token_sort(a), token_sort(b))
  token_set_ratio(a, b)    the shortcut rule of the issue (set_rule), held to token_set_brute -- the maximum of indel over the three
                           pairs built from sect, sect + " " + ab and sect + " " + ba -- by tests/test_token_cpu.py

lcs() is the textbook DP; the frames of the GPU tests take their LCS from indel_ref.batch_numpy_lcs (the same recurrence vectorised
over rows) and the long strings from indel_ref.CRef.
"""
import numpy as np

import indel_ref

WHITESPACE = ([0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
              + list(range(0x09, 0x0E)) + list(range(0x1C, 0x20)) + list(range(0x2000, 0x200B)))


def lcs(a: str, b: str) -> int:
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b, 1):
            cur.append(prev[j - 1] + 1 if x == y else max(prev[j], cur[j - 1]))
        prev = cur
    return prev[len(b)]


def E(d: int, s: int) -> float:
    if s == 0:
        return 1.0
    return 1.0 - (float(d) / float(s))


def indel_distance(a: str, b: str, lcs_fn=lcs) -> int:
    return len(a) + len(b) - 2 * lcs_fn(a, b)


def indel(a: str, b: str, lcs_fn=lcs) -> float:
    return E(indel_distance(a, b, lcs_fn), len(a) + len(b))


def tokens(s: str):
    return s.split()


def token_sort(s: str) -> str:
    return " ".join(sorted(tokens(s)))


def token_sort_ratio(a: str, b: str, lcs_fn=lcs) -> float:
    return indel(token_sort(a), token_sort(b), lcs_fn)


def set_parts(a: str, b: str):
    """(sect, ab, ba): the joined sorted intersection and the two differences of the token SETS."""
    A, B = set(tokens(a)), set(tokens(b))
    return " ".join(sorted(A & B)), " ".join(sorted(A - B)), " ".join(sorted(B - A))


def set_rule(a: str, b: str, lcs_fn=lcs) -> float:
    A, B = set(tokens(a)), set(tokens(b))
    if not A or not B:
        return 0.0
    if (A & B) and (not (A - B) or not (B - A)):
        return 1.0
    sect, ab, ba = set_parts(a, b)
    sl, la, lb = len(sect), len(ab), len(ba)
    sep = 1 if sl > 0 else 0
    sab, sba = sl + sep + la, sl + sep + lb
    r0 = E(indel_distance(ab, ba, lcs_fn), sab + sba)
    if sl == 0:
        return r0
    return max(r0, E(sep + la, sl + sab), E(sep + lb, sl + sba))


token_set_ratio = set_rule


def token_set_brute(a: str, b: str) -> float:
    """The definition: build the three strings and run the textbook DP on the three pairs."""
    A, B = set(tokens(a)), set(tokens(b))
    if not A or not B:
        return 0.0
    sect, ab, ba = set_parts(a, b)
    if sect and (not ab or not ba):
        return 1.0
    c_ab = sect + " " + ab if sect and ab else sect + ab
    c_ba = sect + " " + ba if sect and ba else sect + ba
    r = indel(c_ab, c_ba)
    if sect:
        r = max(r, indel(sect, c_ab), indel(sect, c_ba))
    return r


# ---- whole frames (lists of str) ----

def _frame_indel(X, Y, block=65536):
    out = np.empty(len(X), dtype=np.float64)
    for lo in range(0, len(X), block):
        xs, ys = X[lo:lo + block], Y[lo:lo + block]
        d = indel_ref.batch_numpy_distance(xs, ys)
        for i in range(len(xs)):
            out[lo + i] = E(int(d[i]), len(xs[i]) + len(ys[i]))
    return out


def frame_sort_ratio(A, B):
    return _frame_indel([token_sort(s) for s in A], [token_sort(s) for s in B])


def frame_set_ratio(A, B, block=65536):
    parts = [set_parts(a, b) for a, b in zip(A, B)]
    out = np.empty(len(A), dtype=np.float64)
    for lo in range(0, len(A), block):
        ps = parts[lo:lo + block]
        d = indel_ref.batch_numpy_distance([p[1] for p in ps], [p[2] for p in ps])
        for i, (sect, ab, ba) in enumerate(ps):
            a, b = A[lo + i], B[lo + i]
            if not tokens(a) or not tokens(b):
                out[lo + i] = 0.0
            elif sect and (not ab or not ba):
                out[lo + i] = 1.0
            else:
                sl, la, lb = len(sect), len(ab), len(ba)
                sep = 1 if sl > 0 else 0
                sab, sba = sl + sep + la, sl + sep + lb
                r = E(int(d[i]), sab + sba)
                if sl:
                    r = max(r, E(sep + la, sl + sab), E(sep + lb, sl + sba))
                out[lo + i] = r
    return out


def broadcast(A, B):
    """The library's literal rule: a column of one row is repeated."""
    if len(A) == 1 and len(B) != 1:
        A = A * len(B)
    elif len(B) == 1 and len(A) != 1:
        B = B * len(A)
    return A, B


# ---- the generator of the random frames (issue: 1-4 tokens of 1-6 letters over abcdefgh) ----

def gen_frame(seed, n):
    rng = np.random.default_rng(seed)
    letters = "abcdefgh"

    def tok():
        return "".join(letters[int(k)] for k in rng.integers(0, 8, int(rng.integers(1, 7))))

    def edit(t):
        i = int(rng.integers(0, len(t)))
        op = int(rng.integers(0, 3))
        c = letters[int(rng.integers(0, 8))]
        if op == 0:
            return t[:i] + c + t[i + 1:]
        if op == 1:
            return t[:i] + c + t[i:]
        return (t[:i] + t[i + 1:]) or c

    A, B = [], []
    for _ in range(n):
        ta = [tok() for _ in range(int(rng.integers(1, 5)))]
        if rng.random() < 0.5:
            tb = [edit(t) if rng.random() < 0.4 else t for t in ta]
            rng.shuffle(tb)
            r = rng.random()
            if r < 0.15:
                tb.append(tok())
            elif r < 0.30 and len(tb) > 1:
                tb.pop()
        else:
            tb = [tok() for _ in range(int(rng.integers(1, 5)))]
        A.append(" ".join(ta))
        B.append(" ".join(tb))
    return A, B
