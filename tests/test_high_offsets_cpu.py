"""The geometry of tests/high_offsets.py, on the frames tests/test_high_offsets_gpu.py places: offsets only, no buffer.  Every
placement is monotone as uint32, its int32 bit pattern is negative exactly at and above 2^31, a sign_* placement's row starts below
2^31 and ends above it, the top placements end where they say, and the columns of one call are disjoint with a guard between them."""
import numpy as np
import pytest

import gen
import high_offsets as H
import relation_frames as F


def frames():
    X, Y = F.mixed_frame("levenshtein")
    TX, TY = F.mixed_frame("token_sort_ratio")
    Q, Cs = F.search_frame()
    BQ, BC = gen.batch_boundary_frame(11, "both")
    out = {"pair a": X, "pair b": Y, "token a": TX, "token b": TY, "queries": Q, "candidates": Cs, "slow queries": BQ, "slow candidates": BC}
    out.update({k + " reversed": v[::-1] for k, v in list(out.items())})
    out.update({k + " with an empty last row": v + [""] for k, v in list(out.items()) if "reversed" not in k})
    out["one row"] = ["ab " * 30]
    return out


FRAMES = frames()


def offsets_of(strings, name):
    base, shift = H.Layout().resolve(strings, name)
    assert shift == 0  # (a layout without other columns)
    return H.column_offsets(H.byte_lengths(strings), base)


@pytest.mark.parametrize("name", H.PLACEMENTS)
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_placement_geometry(frame, name):
    strings = FRAMES[frame]
    if frame == "one row" and name == "sign_short":  # (a literal of 90 bytes: no such row)
        with pytest.raises(ValueError):
            H.straddle_row(strings, name)
        return
    off = offsets_of(strings, name)
    lengths = H.byte_lengths(strings)
    wide = off.astype(np.int64)
    assert off.dtype == np.uint32 and off.size == len(strings) + 1
    assert np.array_equal(np.diff(wide), lengths)                      # monotone as uint32, row by row the strings' bytes
    assert 0 <= wide[0] and wide[-1] <= H.TOP
    assert np.array_equal(H.as_int32(off) < 0, wide >= H.SIGN)          # the sign bit: exactly at and above 2^31
    assert np.array_equal(H.as_int32(off).view(np.uint32), off)
    if name == "low":
        assert wide[0] == 0 and (H.as_int32(off) >= 0).all()
    elif name in H.TOPS:
        assert wide[-1] == H.TOPS[name] == {"top1": 0xFFFFFFFF, "top16": 0xFFFFFFF0, "top17": 0xFFFFFFEF}[name]
        assert (H.as_int32(off) < 0).all()
    else:
        r = H.straddle_row(strings, name)
        assert wide[r] < H.SIGN < wide[r + 1]                         # bytes 2^31 - 1 and 2^31 are both the row's
        assert H.as_int32(off)[r] >= 0 > H.as_int32(off)[r + 1]
        raw = strings[r].encode("utf-8")
        if name == "sign_short":
            assert 2 <= len(raw) <= 32 and raw.isascii()
        elif any(len(s.encode("utf-8")) > 128 for s in strings):
            assert len(raw) > 128
        else:
            assert len(raw) == lengths.max()


def test_top16_ends_a_chunk_and_top17_does_not():
    for name, last in (("top1", 0xFFFFFFFE), ("top16", 0xFFFFFFEF), ("top17", 0xFFFFFFEE)):
        off = offsets_of(FRAMES["pair a"], name)
        assert int(off[-1]) - 1 == last                                # the column's last byte
    assert 0xFFFFFFEF % 16 == 15 and 0xFFFFFFEE % 16 == 14 and 0xFFFFFFFE % 16 == 14


def test_a_column_past_the_last_offset_is_refused():
    with pytest.raises(ValueError):
        H.column_offsets([10, 10], H.TOP - 19)
    assert int(H.column_offsets([10, 10], H.TOP - 20)[-1]) == H.TOP


@pytest.mark.parametrize("variant", ["", " reversed", " with an empty last row"])
@pytest.mark.parametrize("pa,pb", H.PAIRS + (("low", "low"),))
@pytest.mark.parametrize("fa,fb", [("pair a", "pair b"), ("token a", "token b"), ("queries", "candidates"), ("slow queries", "slow candidates")])
def test_columns_of_one_call_are_disjoint(fa, fb, pa, pb, variant):
    A, B = FRAMES[fa + variant], FRAMES[fb + variant]
    lay = H.Layout()
    spans = []
    for strings, name in ((A, pa), (B, pb)):
        base, shift = lay.resolve(strings, name)
        nbytes = int(H.byte_lengths(strings).sum())
        lay.claim(shift + base, nbytes)
        off = H.column_offsets(H.byte_lengths(strings), base)
        if name.startswith("sign"):  # shifted or not, the offsets cross the sign bit inside the chosen row
            r = H.straddle_row(strings, name)
            assert int(off[r]) < H.SIGN < int(off[r + 1])
        spans.append((shift + base, shift + base + nbytes, shift))
    (s0, e0, sh0), (s1, e1, sh1) = spans
    assert e0 + H.GUARD <= s1 or e1 + H.GUARD <= s0                      # disjoint, and neither inside the other's guard
    assert 0 <= min(s0, s1) and max(e0, e1) + H.GUARD <= H.SIZE          # the guards too lie inside the buffer
    assert sh0 == 0 and sh1 == (H.SHIFT if (pa, pb) == ("sign_long", "sign_short") else 0)
    if (pa, pb) == ("low", "low"):
        assert s0 == 0 and s1 % H.GUARD == 0 and s1 >= e0 + H.GUARD


def test_layout_refuses_overlap_and_the_outside():
    lay = H.Layout()
    lay.claim(10 * H.GUARD, 100)
    for start in (10 * H.GUARD + 50, 9 * H.GUARD + 1, 10 * H.GUARD + 100 + H.GUARD - 1):
        with pytest.raises(ValueError):
            lay.claim(start, 100)
    lay.claim(10 * H.GUARD + 100 + H.GUARD, 100)
    with pytest.raises(ValueError):
        H.Layout().claim(H.SIZE - 10, 11)
    with pytest.raises(ValueError):
        H.Layout().claim(-1, 4)


def test_poison_pattern():
    assert len(H.POISON) == 4 and H.POISON[0] >= 0x80 and chr(H.POISON[1]).isalpha() and H.POISON[2] & 0xC0 == 0x80 and H.POISON[3] == 0x20
    assert H.SIZE == 2 ** 32 + 2 ** 21 and H.SIZE % 4 == 0
