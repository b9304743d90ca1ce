"""The frames of the block-cut tests, built once each and cached, the block cut of the staged lane kernels restated in plain Python,
and the builder of the frames whose first block fits its staging area exactly or misses it by one byte.

Every frame is ASCII (one byte per character), so lengths in characters are lengths in bytes.  A frame's column lies in its value
buffer as tests/test_stage_cut_gpu.py lays it out: the buffer the kernel sees starts `shift` bytes behind a 16-byte boundary (junk
bytes fill the gap), then come `base` junk bytes that belong to the buffer (offsets[0] == base), the strings, and 64 readable
zero bytes.

The restated rule (blocks, late_rows) follows strsim_lane_stage.h (lane_stage_body: the ranges of grab(), the block cut, the `mine`
test of sortA) and strsim_lane_lit.h (the workgroup's range, cut(), the `fast` test) line by line in what it decides and shares no
code with either.
"""
import functools
import random
import zlib
from collections import namedtuple

import numpy as np

import gen
import oracle_lib as O

CHUNK = 64          # rows per chunk: the unit of the cut
BLOCK_ROWS = 512    # rows per block, at most (STRSIM_STAGE_ROWS, LIT_ROWS)
CAP_PLAIN = 10240   # STRSIM_STAGE_CAP
CAP_TABLES = 8960   # STRSIM_STAGE_CAP_LUT
CAP_LONG = 15104    # STRSIM_STAGE_CAP_LONG
CAP_LIT = 10240     # LIT_CAP
MAX_ROWS = 4160     # the frames here are small: see ranges()
JUNK = 0xE9         # what lies in front of a column's first string: a byte that would make a row non-ASCII if it were read as text

ROWS = 4096
LITERAL = "kitten"
LITERALS = ["", "abcdefghijklmnopqrstuvwxyzabcdef", "kitten"]

Frame = namedtuple("Frame", "name A B shifts bases")  # A, B: tuples of str; shifts, bases: (column a, column b)
Block = namedtuple("Block", "row0 rows chunks spans staged mis")  # spans, staged, mis: per column side, None for a literal side


# ---- the existing frames ------------------------------------------------------------------------------------------------------------
def partner(rng, a, lo, hi):
    r = rng.random()
    b = gen.edit(rng, a, gen.ASCII_LOWER, rng.randint(1, 3)) if r < 0.5 else (a if r < 0.55 else gen.rand_string(rng, gen.ASCII_LOWER, lo, hi))
    b = b[:hi]
    while len(b) < lo:
        b += rng.choice(gen.ASCII_LOWER)
    return b


def _law(seed, n, lo, hi):
    rng = random.Random(seed)
    A = [gen.rand_string(rng, gen.ASCII_LOWER, lo, hi) for _ in range(n)]
    B = [partner(rng, a, lo, hi) for a in A]
    return A, B


def _one_chunk(at, rows_a, rows_b):
    """frame (a) with the 64 rows from `at` on replaced"""
    A, B = _law(31, ROWS, 0, 32)
    assert len(rows_a) == len(rows_b) == CHUNK
    A[at:at + CHUNK], B[at:at + CHUNK] = rows_a, rows_b
    return A, B


def _build(name):
    if name == "a":  # full blocks: U{0..32} on both sides, 4 096 rows
        return _law(31, ROWS, 0, 32)
    if name == "b":  # every block cut, in every geometry: 28..32 bytes on both sides (512 rows are 15 360 bytes)
        return _law(32, ROWS, 28, 32)
    if name == "c":  # cuts of changing length, either column deciding: runs of 200 rows of 30..32-byte and of 0..4-byte strings
        rng = random.Random(33)
        A, B = [], []
        for i in range(4160):
            run = (i // 200) % 4
            la, lb = ((30, 32), (30, 32)) if run == 0 else ((0, 4), (0, 4)) if run == 1 else ((30, 32), (0, 4)) if run == 2 else ((0, 4), (30, 32))
            A.append(gen.rand_string(rng, gen.ASCII_LOWER, *la))
            B.append(gen.rand_string(rng, gen.ASCII_LOWER, *lb) if run >= 2 or rng.random() < 0.5 else partner(rng, A[-1], *lb))
        return A, B
    if name.startswith("d"):  # small frames: one block that is not full; a one-row last block; a last block of a single chunk
        n = int(name[1:])
        return _law(34 + n, n, 0, 32)
    if name == "e":  # the chunk that overflows alone (10 240 and 8 960; the long geometry holds it): 64 rows of 200 bytes
        rng = random.Random(35)
        a, b = [], []
        for _ in range(CHUNK):
            a.append(gen.rand_string(rng, gen.ASCII_LOWER, 200, 200))
            b.append(gen.edit(rng, a[-1], gen.ASCII_LOWER, 3)[:200])
        return _one_chunk(2048 + CHUNK, a, b)
    if name in ("e_long_first", "e_long_last"):
        # a chunk that overflows every staging area alone: 48 rows of 400 bytes (19 200) and 16 rows of 10 bytes.  Long rows first:
        # the 10-byte rows are lane class but lie beyond the staged bytes.  Long rows last: the 10-byte rows are staged and computed.
        rng = random.Random(36 if name == "e_long_first" else 37)
        la, sa, lb, sb = [], [], [], []
        for _ in range(48):
            la.append(gen.rand_string(rng, gen.ASCII_LOWER, 400, 400))
            lb.append(gen.edit(rng, la[-1], gen.ASCII_LOWER, 3)[:400])
        for _ in range(16):
            sa.append(gen.rand_string(rng, gen.ASCII_LOWER, 10, 10))
            sb.append(partner(rng, sa[-1], 10, 10))
        if name == "e_long_first":
            return _one_chunk(2048 + CHUNK, la + sa, lb + sb)
        return _one_chunk(2048 + CHUNK, sa + la, sb + lb)
    raise KeyError(name)


FRAME_NAMES = ["a", "b", "c", "d70", "d1025", "d1088", "e", "e_long_first", "e_long_last", "g1", "g7", "g15"]


_EDGE_BY_NAME = {}


@functools.lru_cache(maxsize=None)
def frame(name):
    """the frame of that name; built once, never changed"""
    if name in _EDGE_BY_NAME:
        return _EDGE_BY_NAME[name]
    if name.startswith("g"):  # frame (a) with misaligned value buffers: column a `shift` bytes behind a 16-byte boundary, column b 16 - shift
        shift = int(name[1:])
        f = frame("a")
        return Frame(name, f.A, f.B, (shift, 16 - shift), (0, 0))
    if name == "primer":
        return _primer()
    A, B = _build(name)
    assert len(A) == len(B) <= MAX_ROWS
    return Frame(name, tuple(A), tuple(B), (0, 0), (0, 0))


def _primer():
    """1 024 rows of frame (a)'s law; every eighth row is a 40-byte ASCII string against an edited copy: 128 rows for the later kernels"""
    rng = random.Random(38)
    A, B = _law(39, 1024, 0, 32)
    for i in range(0, 1024, 8):
        A[i] = gen.rand_string(rng, gen.ASCII_LOWER, 40, 40)
        B[i] = gen.edit(rng, A[i], gen.ASCII_LOWER, 2)
    return Frame("primer", tuple(A), tuple(B), (0, 0), (0, 0))


def sides(f, literal_side=None, literal=LITERAL):
    """(A, B) of a call: the frame's columns, or its column against a one-row side (literal_side 'a': the literal is side a and the
    column is the frame's B)"""
    if literal_side is None:
        return f.A, f.B
    return ((literal,), f.B) if literal_side == "a" else (f.A, (literal,))


@functools.lru_cache(maxsize=None)
def expected(name, measure, literal_side=None, literal=LITERAL):
    """the oracle's column for a call of the frame of that name (cached per frame, measure and literal; read-only)"""
    f = frame(name)
    A, B = sides(f, literal_side, literal)
    exp = O.batch_strings(measure, list(A), list(B), 8)
    exp.setflags(write=False)
    return exp


# ---- the layout of a column -----------------------------------------------------------------------------------------------------------
def offsets(strings, base=0):
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return off + base


def column_bytes(strings, shift=0, base=0):
    """(offsets u32, buffer u8): the column's value buffer is buffer[shift:]; put buffer at a 16-byte boundary"""
    text = "".join(strings).encode("ascii")
    buf = np.concatenate([np.full(shift + base, JUNK, dtype=np.uint8), np.frombuffer(text, dtype=np.uint8), np.zeros(64, dtype=np.uint8)])
    return offsets(strings, base).astype(np.uint32), buf


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------
def ranges(n, kind):
    """row ranges [lo, hi) that one workgroup walks block by block; a block never crosses one"""
    assert 0 < n <= MAX_ROWS
    nchunks = -(-n // CHUNK)
    if kind == "lit":
        # launch_lane_t: min(ceil(n / LIT_ROWS), 3 x the resident workgroups) workgroups, each ceil(nchunks / workgroups) chunks
        groups = -(-n // BLOCK_ROWS)
        per = -(-nchunks // groups)
    else:
        # grab(): what is left / (4 x workgroups), at least two blocks; stage_launch_size gives a frame of up to MAX_ROWS rows one
        # workgroup per block, so the quotient is at most 2 and a range is two blocks' chunks
        assert kind == "stage"
        per = 2 * BLOCK_ROWS // CHUNK
    return [(lo * CHUNK, min((lo + per) * CHUNK, n)) for lo in range(0, nchunks, per)]


def blocks(off_a, off_b, shift_a, shift_b, cap, n, kind, fit=None):
    """The blocks a call of n rows is cut to.  off_x: the offsets of a column side, None for a one-row side (it is not staged);
    shift_x: the address of the value buffer modulo 16.  A block takes the chunks c = 0, 1, .. while
    end - base + mis <= cap holds for both columns behind chunk c, and at least one.  `fit` replaces the comparison (the mutation
    checks of tests/test_stage_frames_cpu.py)."""
    fit = fit or (lambda span, cap_: span <= cap_)
    cols = [(off, shift) for off, shift in ((off_a, shift_a), (off_b, shift_b))]
    out = []
    for lo, hi in ranges(n, kind):
        row = lo
        while row < hi:
            avail = min(hi - row, BLOCK_ROWS)
            mis = [None if off is None else int(shift + off[row]) % 16 for off, shift in cols]

            def spans(e):
                return [None if off is None else int(off[row + e] - off[row]) + m for (off, _), m in zip(cols, mis)]
            k = 0
            while k * CHUNK < avail and k < BLOCK_ROWS // CHUNK:
                e = min((k + 1) * CHUNK, avail)
                if not all(s is None or fit(s, cap) for s in spans(e)):
                    break
                k += 1
            k = max(k, 1)
            rows = min(k * CHUNK, avail)
            sp = spans(rows)
            staged = [None if s is None else (min(s, cap) + 15) & ~15 for s in sp]
            out.append(Block(row, rows, k, tuple(sp), tuple(staged), tuple(mis)))
            row += rows
    return out


def late_rows(blks, off_a, off_b, lit_len=None):
    """Rows the first kernel leaves to the later ones: a string longer than 32 bytes, or one that does not lie inside the staged
    bytes of its block (mis + start + length <= staged).  lit_len: the length of the one-row side, if there is one."""
    if lit_len is not None and lit_len > 32:
        return sum(b.rows for b in blks)
    late = 0
    for b in blks:
        for i in range(b.row0, b.row0 + b.rows):
            ok = True
            for off, staged, mis in zip((off_a, off_b), b.staged, b.mis):
                if off is None:
                    continue
                start, length = int(off[i] - off[b.row0]), int(off[i + 1] - off[i])
                ok = ok and length <= 32 and mis + start + length <= staged
            late += not ok
    return late


def call_blocks(f, cap, kind, literal_side=None, fit=None):
    """blocks() of a call of frame f: both columns, or the column that stands against a one-row side"""
    off_a = None if literal_side == "a" else offsets(f.A, f.bases[0])
    off_b = None if literal_side == "b" else offsets(f.B, f.bases[1])
    return blocks(off_a, off_b, f.shifts[0], f.shifts[1], cap, len(f.A), kind, fit), off_a, off_b


def call_late_rows(f, cap, kind, literal_side=None, literal=LITERAL):
    blks, off_a, off_b = call_blocks(f, cap, kind, literal_side)
    return late_rows(blks, off_a, off_b, None if literal_side is None else len(literal))


# ---- edge frames ------------------------------------------------------------------------------------------------------------------------
# chunks of the first block and the bytes of each: full chunks of 64 equal-sized-on-average rows, then the chunk that ends the block
EDGE_SHAPE = {CAP_PLAIN: (5, 1792, 1280), CAP_TABLES: (4, 1792, 1792), CAP_LONG: (7, 2048, 768)}
EDGE_ROWS = 1100  # three blocks' worth: two ranges of the stage kernel, three workgroups of six chunks of the literal kernel


def edge_chunks(cap):
    """k: the number of chunks behind which the deciding column's span is cap + delta"""
    return EDGE_SHAPE[cap][0] + 1


def _lengths(rng, total, lo=0, hi=32):
    """64 lengths in lo..hi that add up to total"""
    assert CHUNK * lo <= total <= CHUNK * hi
    ls = [total // CHUNK + (1 if i < total % CHUNK else 0) for i in range(CHUNK)]
    for _ in range(4 * CHUNK):  # move single bytes between rows
        i, j = rng.randrange(CHUNK), rng.randrange(CHUNK)
        if i != j and ls[i] < hi and ls[j] > lo:
            ls[i] += 1
            ls[j] -= 1
    assert sum(ls) == total
    return ls


@functools.lru_cache(maxsize=None)
def edge_frame(cap, decider, delta, mis, base):
    """About 1 100 rows whose first block is decided by one byte.  The deciding column's span behind chunk k = edge_chunks(cap)
    -- its bytes plus the misalignment of its first string, (mis + base) % 16 -- is cap + delta; behind chunk k - 1 it is at
    least 700 bytes less.  The other column holds edited copies of the first half of each string.  The value buffers start `mis`
    bytes behind a 16-byte boundary and `base` junk bytes lie in front of the first string (offsets[0] == base).  The rows behind
    the first block follow frame (a)'s law."""
    full, full_bytes, last_bytes = EDGE_SHAPE[cap]
    assert decider in ("a", "b") and 0 <= mis < 16
    rng = random.Random(zlib.crc32(repr(("edge", cap, decider, delta, mis, base)).encode()))
    first = (mis + base) % 16
    ls = []
    for _ in range(full):
        ls += _lengths(rng, full_bytes, full_bytes // CHUNK - 4, 32)
    ls += _lengths(rng, last_bytes - first + delta)
    D = [gen.rand_string(rng, gen.ASCII_LOWER, l, l) for l in ls]
    other = [gen.edit(rng, d[:len(d) // 2], gen.ASCII_LOWER, rng.randint(1, 3))[:32] for d in D]
    TA, TB = _law(rng.randrange(1 << 16), EDGE_ROWS - len(D), 0, 32)
    A, B = (D + TA, other + TB) if decider == "a" else (other + TA, D + TB)
    f = Frame("edge_%d_%s_%+d_%d_%d" % (cap, decider, delta, mis, base), tuple(A), tuple(B), (mis, mis), (base, base))
    _EDGE_BY_NAME[f.name] = f
    return f


def check_edge_frame(f, cap, kind, decider, delta, literal_side=None, fit=None):
    """The builder's promise, by the restated rule: the first block holds k chunks for delta <= 0 and k - 1 for + 1, the named column
    decides, and its span behind chunk k is cap + delta.  -> the blocks"""
    k = edge_chunks(cap)
    d = 0 if decider == "a" else 1
    blks, off_a, off_b = call_blocks(f, cap, kind, literal_side, fit)
    b0 = blks[0]
    assert b0.row0 == 0 and all(max(len(s) for s in X) <= 32 for X in (f.A, f.B))
    offs = (off_a, off_b)
    span_k = [None if off is None else int(off[k * CHUNK] - off[0]) + b0.mis[i] for i, off in enumerate(offs)]
    assert span_k[d] == cap + delta, (span_k, cap, delta)
    assert int(offs[d][(k - 1) * CHUNK] - offs[d][0]) + b0.mis[d] <= cap - 700
    if span_k[1 - d] is not None:  # the other column is at least a chunk's worth below its cap: it never decides
        assert span_k[1 - d] <= cap - 2048, span_k
    assert b0.chunks == (k if delta <= 0 else k - 1), (b0, k, delta)
    if delta <= 0 and k < BLOCK_ROWS // CHUNK and b0.rows == k * CHUNK:
        # ... and it is the cap that ends the block, where neither the block size nor the range does: the next chunk does not fit
        nxt = min((k + 1) * CHUNK, len(f.A))
        rng_hi = [hi for lo, hi in ranges(len(f.A), kind) if lo == 0][0]
        if rng_hi > k * CHUNK:
            assert int(offs[d][min(nxt, rng_hi)] - offs[d][0]) + b0.mis[d] > cap
    return blks
