"""The frames both relation suites run on (tests/test_relations_cpu.py: the models, tests/test_relations_gpu.py: the kernels): fixed
seeds of tests/relations.py's generator, each built once."""
import functools
import random

import relations as T
from token_ref import WHITESPACE

WS_ALL = "".join(chr(c) for c in WHITESPACE)            # Python's str.isspace set, 29 code points
WS_ASCII = "".join(c for c in WS_ALL if ord(c) < 0x80)  # 0x09 .. 0x0D, 0x1C .. 0x20
PAD = "abcdef"                                          # what common affixes are made of
N = 3000                                                # pairs of a relation (2 000 .. 4 000)
N_LONG = 300                                            # pairs of the 1 024 / 1 025-byte affix cases
SEARCH_KS = (1, 3, 16)


@functools.lru_cache(maxsize=None)
def pair_frame(seed=1, n=N):
    return T.frame(seed, n)


@functools.lru_cache(maxsize=None)
def token_frame(seed=2, n=N):
    return T.token_frame(seed, n)


@functools.lru_cache(maxsize=None)
def padded_frame(longest, n):
    """pair_frame's first n pairs with random common affixes, the longer string of every pair exactly `longest` bytes."""
    A, B = pair_frame()
    return T.pad_columns_to(longest, A[:n], B[:n], longest, PAD)


@functools.lru_cache(maxsize=None)
def equal_length_frame(seed=3, n=N):
    """Pairs of equal length: a random string and a copy with substitutions and adjacent swaps."""
    rng = random.Random(seed)
    A, B = [], []
    for i in range(n):
        al = T.ALPHABETS[i % 2]
        a = "".join(rng.choice(al) for _ in range(rng.randint(1, T.BASE_MAX_LEN)))
        b = list(a) if rng.random() < 0.7 else [rng.choice(al) for _ in a]
        for _ in range(rng.randint(0, 4)):
            p = rng.randrange(len(b))
            if rng.random() < 0.5 or p + 1 == len(b):
                b[p] = rng.choice(al)
            else:
                b[p], b[p + 1] = b[p + 1], b[p]
        A.append(a)
        B.append("".join(b))
    return A, B


HAYSTACK_LENGTHS = (24, 31, 32, 33, 34, 48)  # both sides of the 32-byte lane cap of the partial ratio


@functools.lru_cache(maxsize=None)
def contained_frame(seed=4, n=N):
    """(needles, haystacks): a non-empty needle of up to 20 characters inside x + a + y of HAYSTACK_LENGTHS characters."""
    rng = random.Random(seed)
    needles, hay = [], []
    for i in range(n):
        al = T.ALPHABETS[i % 2]
        a = "".join(rng.choice(al) for _ in range(rng.randint(1, 20)))
        x, y = T.pad_pair_to(rng, a, a, rng.choice(HAYSTACK_LENGTHS), al)
        assert x == y
        needles.append(a)
        hay.append(x)
    return needles, hay


@functools.lru_cache(maxsize=None)
def token_images(mode, side):
    """token_frame with one side's tokens permuted (relation_checks.token_image): "spread" and "copies" use ASCII whitespace, so the
    image leaves the lane tier by its length or token count alone; "unicode" uses all 29 whitespace characters."""
    import relation_checks as RC
    A, B = token_frame()
    ws = WS_ALL if mode == "unicode" else WS_ASCII
    if side == "a":
        return RC.token_image(5, A, ws, mode), B
    return A, RC.token_image(6, B, ws, mode)


@functools.lru_cache(maxsize=None)
def search_frame(nq=128, nc=300):
    return T.search_frame(7, nq, nc)


@functools.lru_cache(maxsize=None)
def token_search_frame(nq=128, nc=300):
    return T.token_search_frame(8, nq, nc)


def frame_of(m):
    import relation_checks as RC
    return token_frame() if m in RC.TOKEN else pair_frame()


def mixed_frame(m):
    """Rows of every tier in one frame: lane class, 2- and 4-byte relabelled, padded to 65 and 129 bytes, and a few beyond WAVE_CAP."""
    A, B = frame_of(m)
    X, Y = A[:1500], B[:1500]
    X += [T.relabel(s, 0x400) for s in A[1500:2000]] + [T.relabel(s, 0x1F600) for s in A[2000:2500]]
    Y += [T.relabel(s, 0x400) for s in B[1500:2000]] + [T.relabel(s, 0x1F600) for s in B[2000:2500]]
    for longest, n in ((65, 300), (129, 300), (1025, 40)):
        P, Q = padded_frame(longest, n)
        X, Y = X + P, Y + Q
    return X, Y


SEARCH_PREFIX = "x" * 33  # one byte past the 32-byte lane class of the searches
# cutoffs that drop some candidates of a query and keep others (test_relations_cpu.py asserts that on the models)
NEAREST_CUTOFF = 3
EXTRACT_CUTOFF = {"indel": 0.6, "token_sort_ratio": 0.6}
BEST_MATCH_CUTOFF = {"levenshtein": 0.5, "jaro": 0.7, "jaro_winkler": 0.7, "jaccard": 0.4, "sorensen_dice": 0.5}
