"""Placements of a column anywhere in the first 4 GiB behind its values pointer (include/strsim_amd.h: "any monotone base is
accepted", "Nothing outside [a_offsets[0], a_offsets[a_rows]) can change a result"), for tests/test_high_offsets_gpu.py.

The geometry is plain integer arithmetic and needs neither a GPU nor memory (tests/test_high_offsets_cpu.py holds it to its rules):

  column_offsets(lengths, base)   the uint32 offsets of a column whose first byte is `base`
  as_int32(offsets)               the same bits as int32, as strsim_amd.Context takes device offsets (torch has no uint32 arithmetic)
  straddle_row(strings, name)     the row a sign_* placement puts byte 2^31 into
  named_base(strings, name)       where a named placement puts the column's first byte
  Layout                          the regions of one call: inside the buffer, and no region inside another's guard

Named placements (T: the column's byte size):

  low         base 0, the control (a second low column of the same call: the first free 4 KiB boundary behind the others)
  sign_short  byte 2^31 strictly inside a row of 2 .. 32 ASCII bytes: the row starts below 2^31 and ends above it
  sign_long   the same inside a row of more than 128 bytes (beyond every lane tier); a frame without one: inside its longest row
  top1        offsets[rows] == 2^32 - 1, the largest offset there is
  top16       offsets[rows] == 2^32 - 16: the column's last byte ends a 16-byte chunk
  top17       offsets[rows] == 2^32 - 17

HighBuffer is the memory: ONE uint8 tensor of 2^32 + 2^21 bytes on the device (the 2 MiB behind byte 2^32 - 1 keep a small
over-read by a wrapped bound inside the allocation, where it shows as a wrong result or counter and not as a fault), filled once with
POISON -- a byte with its high bit set, a letter, a continuation byte and a space, so that a byte leaked from outside a column
either changes a score or sends the row to a slower tier.  place() writes a column's bytes, poisons 4 KiB on either side of them
again (an earlier call's column may have lain there) and returns (offsets, values) as the device entry points take them.  The
values tensor is the whole buffer, its data_ptr() byte 0 -- with one exception: byte 2^31 of one address space cannot lie inside
two disjoint columns, so the second sign_* column of a call is placed SHIFT bytes further up and its values tensor is the
buffer from byte SHIFT on; its offsets straddle 2^31 all the same.
"""
import numpy as np

SIGN = 2 ** 31
TOP = 2 ** 32 - 1                    # the largest uint32 offset
SLACK = 2 ** 21
SIZE = 2 ** 32 + SLACK
GUARD = 4096                         # bytes poisoned again on either side of a placed column
SHIFT = 2 ** 20                      # where the values tensor of a call's second sign_* column begins
POISON = bytes((0xFF, 0x61, 0x80, 0x20))
MIN_FREE = 8 * 2 ** 30               # free device memory below which the module is skipped

PLACEMENTS = ("low", "sign_short", "sign_long", "top1", "top16", "top17")
TOPS = {"top1": TOP, "top16": 2 ** 32 - 16, "top17": 2 ** 32 - 17}
# (placement of column a, placement of column b) of a two-column call
PAIRS = (("sign_short", "top1"), ("top1", "sign_long"), ("top16", "low"), ("low", "top17"), ("sign_long", "sign_short"))
SHORT_MAX, LONG_MIN = 32, 129        # a sign_short row has at most / a sign_long row at least this many bytes


def encode(strings):
    return [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strings]


def byte_lengths(strings):
    return np.array([len(b) for b in encode(strings)], dtype=np.int64)


def column_offsets(lengths, base):
    """uint32 [rows + 1]: offsets[0] = base, offsets[i + 1] = offsets[i] + lengths[i]; the last one is at most 2^32 - 1."""
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    off[0] = base
    off[1:] = base + np.cumsum(np.asarray(lengths, dtype=np.int64))
    if base < 0 or int(off[-1]) > TOP:
        raise ValueError(f"a column of {int(off[-1]) - base} bytes at base {base} does not fit 32-bit offsets")
    return off.astype(np.uint32)


def as_int32(offsets):
    return np.ascontiguousarray(offsets, dtype=np.uint32).view(np.int32)


def straddle_row(strings, name):
    """The row of a sign_* placement: the suitable one nearest the middle of the column."""
    raw = encode(strings)
    n = len(raw)
    if name == "sign_short":
        ok = [2 <= len(b) <= SHORT_MAX and max(b) < 0x80 for b in raw]
    elif name == "sign_long":
        ok = [len(b) >= LONG_MIN for b in raw]
        if not any(ok):
            longest = max(len(b) for b in raw)
            ok = [len(b) == longest and longest >= 2 for b in raw]
    else:
        raise ValueError(name)
    rows = [i for i in range(n) if ok[i]]
    if not rows:
        raise ValueError(f"no row for {name} among {n}")
    return min(rows, key=lambda i: (abs(i - n // 2), i))


def straddle_base(lengths, row):
    """The base that puts byte 2^31 into the middle of `row` (at least one of its bytes on either side)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    if lengths[row] < 2:
        raise ValueError("a straddled row needs two bytes")
    return SIGN - int(lengths[:row].sum()) - int(lengths[row]) // 2


def named_base(strings, name):
    """The first byte of the column under a placement other than low (whose base is the layout's to give)."""
    lengths = byte_lengths(strings)
    if name in TOPS:
        return TOPS[name] - int(lengths.sum())
    return straddle_base(lengths, straddle_row(strings, name))


class Layout:
    """The byte ranges the columns of one call occupy in the buffer, in the buffer's own coordinates."""

    def __init__(self, size=SIZE):
        self.size, self.regions = size, []

    def reset(self):
        self.regions = []

    def free(self, start, nbytes):
        """Does [start, start + nbytes) lie inside the buffer, outside every region and outside every region's guard?"""
        if start < 0 or start + nbytes > self.size:
            return False
        return all(start + nbytes + GUARD <= s or e + GUARD <= start for s, e in self.regions)

    def claim(self, start, nbytes):
        if not self.free(start, nbytes):
            raise ValueError(f"[{start}, {start + nbytes}) is outside the buffer or within {GUARD} bytes of {self.regions}")
        self.regions.append((start, start + nbytes))
        return start

    def low_base(self, nbytes):
        """Base 0, or the first 4 KiB boundary behind the regions there are at which the column is free."""
        base = 0
        while not self.free(base, nbytes):
            base = min(e for s, e in self.regions if e + GUARD > base) + GUARD
            base = (base + GUARD - 1) // GUARD * GUARD
        return base

    def resolve(self, strings, name):
        """-> (base, shift): the column's offsets start at `base` behind a values pointer `shift` bytes into the buffer."""
        nbytes = int(byte_lengths(strings).sum())
        if name == "low":
            return self.low_base(nbytes), 0
        base = named_base(strings, name)
        shift = 0 if name in TOPS or self.free(base, nbytes) else SHIFT
        return base, shift


class HighBuffer:
    """The 4 GiB buffer on one device; one per test module (close() frees it)."""

    def __init__(self, torch, device):
        self.torch, self.device = torch, device
        self.buf = torch.empty(SIZE, dtype=torch.uint8, device=device)
        self.buf.view(torch.int32).fill_(int(np.frombuffer(POISON, dtype=np.int32)[0]))
        self.layout = Layout()

    def close(self):
        self.buf = None
        self.torch.cuda.empty_cache()

    def reset(self):
        """A new call: its columns may lie where an earlier call's lay."""
        self.layout.reset()

    def _poison(self, start, end):
        start, end = max(start, 0), min(end, SIZE)
        if start < end:
            pat = np.frombuffer(POISON * ((end - start) // 4 + 2), dtype=np.uint8)[start % 4:start % 4 + end - start]
            self.buf[start:end] = self.torch.from_numpy(pat.copy()).to(self.device)

    def place(self, strings, end=None, straddle=None, base=None, shift=0):
        """The packed bytes of `strings` into the buffer -> (offsets int32 tensor [rows + 1], values uint8 tensor).  end: the value
        of offsets[rows]; straddle: the row that holds byte 2^31; base: offsets[0] itself; none of them: base 0.  shift: the values
        tensor is the buffer from that byte on."""
        raw = encode(strings)
        lengths = np.array([len(b) for b in raw], dtype=np.int64)
        nbytes = int(lengths.sum())
        if end is not None:
            base = int(end) - nbytes
        elif straddle is not None:
            base = straddle_base(lengths, straddle)
        elif base is None:
            base = 0
        offsets = column_offsets(lengths, base)
        at = self.layout.claim(shift + base, nbytes)
        if nbytes:
            self.buf[at:at + nbytes] = self.torch.from_numpy(np.frombuffer(b"".join(raw), dtype=np.uint8).copy()).to(self.device)
        self._poison(at - GUARD, at)
        self._poison(at + nbytes, at + nbytes + GUARD)
        return self.torch.from_numpy(as_int32(offsets).copy()).to(self.device), (self.buf[shift:] if shift else self.buf)

    def place_named(self, strings, name):
        base, shift = self.layout.resolve(strings, name)
        return self.place(strings, base=base, shift=shift)
