"""The frame of the wave-kernel route tests (tests/wave_frames.py) holds what its classes claim, from the strings alone: no GPU.

tests/test_wave_routes_gpu.py runs the frame on the device; here every class is checked for the byte lengths, the ASCII-ness, the
scalar-value counts and the BMP membership that put its rows on the route it is named for.
"""
import wave_frames as W

CAP = W.WAVE_CAP


def _rows(name):
    f = W.frame()
    return [(f.A[i], f.B[i]) for i in f.classes[name]]


def _short_long(a, b, size=len):
    return (a, b) if size(a) <= size(b) else (b, a)


def test_frame_is_small_and_every_row_is_left_to_the_wave_kernel():
    f = W.frame()
    assert len(f.A) == len(f.B) <= 512
    assert sorted(i for r in f.classes.values() for i in r) == list(range(len(f.A)))  # the classes partition the frame
    for a, b in zip(f.A, f.B):
        assert max(W.nbytes(a), W.nbytes(b)) > 128
    assert W.frame() is f  # built once


def test_literals():
    assert W.LITERALS["ascii"].isascii() and W.nbytes(W.LITERALS["ascii"]) == 200
    lit = W.LITERALS["cyrillic"]
    assert len(lit) == 100 and W.nbytes(lit) == 200 and all(0x0400 <= ord(c) <= 0x04FF for c in lit)


def test_ascii_classes_hold_every_pattern_size_on_either_side():
    for name, planes in (("ascii_lower", 5), ("ascii_mixed", 7)):
        rows = _rows(name)
        assert all(a.isascii() and b.isascii() for a, b in rows)
        for side in (0, 1):  # the pattern in column a (even rows of the class) / in column b (odd rows)
            mine = rows[side::2]
            assert [len(r[side]) for r in mine] == W.PATTERN_SIZES and all(len(r[side]) <= len(r[1 - side]) for r in mine)
        for a, b in rows:
            s, l = _short_long(a, b)
            assert 129 <= len(l) <= CAP and 1 <= len(s) <= CAP
        # a-z alone: bits 5 and 6 are the same in every byte; mixed case and punctuation: they are not
        differ = {W.vary(a, b) & 0x60 != 0 for a, b in rows if min(len(a), len(b)) > 1}
        assert differ == {planes == 7}, (name, differ)


def test_ascii_against_non_ascii():
    rows = _rows("ascii_vs_non_ascii")
    assert len(rows) >= 4
    for a, b in rows:
        assert a.isascii() != b.isascii() and W.in_bmp(a + b)
        assert max(W.nbytes(a), W.nbytes(b)) <= CAP and min(len(a), len(b)) >= 1
    assert {a.isascii() for a, b in rows} == {True, False}  # the ASCII string on either side


def test_symbol_classes():
    # the bits that differ inside a pair: below bit 7 / below bit 11 / bit 11 or above -> 7, 11, 16 planes
    want = {"cyrillic": lambda v: v < 1 << 7, "latin_cyrillic": lambda v: 1 << 7 <= v < 1 << 11, "mixed": lambda v: v >= 1 << 11, "cjk": lambda v: v >= 1 << 11}
    for name, ok in want.items():
        rows = _rows("symbols_" + name)
        for side in (0, 1):
            mine = rows[side::2]
            assert [len(r[side]) for r in mine] == W.SYMBOL_SIZES and all(len(r[side]) < len(r[1 - side]) for r in mine)
        for a, b in rows:
            assert not a.isascii() and not b.isascii() and W.in_bmp(a + b)
            assert 33 <= max(len(a), len(b)) <= CAP and max(W.nbytes(a), W.nbytes(b)) <= CAP
            assert ok(W.vary(a, b)), (name, hex(W.vary(a, b)))
    assert all(0x4E00 <= ord(c) <= 0x9FFF for a, b in _rows("symbols_cjk") for c in a + b)
    assert all(0x0430 <= ord(c) <= 0x044F for a, b in _rows("symbols_cyrillic") for c in a + b)


def test_beyond_bmp_empty_side_and_the_two_long_classes():
    for a, b in _rows("beyond_bmp"):
        assert not W.in_bmp(a + b) and max(len(a), len(b)) > 32 and min(len(a), len(b)) >= 1
        assert max(W.nbytes(a), W.nbytes(b)) <= CAP
    rows = _rows("empty_side")
    assert {(a == "", b == "") for a, b in rows} == {(True, False), (False, True)}
    assert all(128 < W.nbytes(a + b) <= CAP for a, b in rows)
    assert {(a + b).isascii() for a, b in rows} == {True, False}
    # more than 1 024 bytes but at most 1 024 values, inside the BMP: Levenshtein's symbol route
    rows = _rows("symbol_route")
    for a, b in rows:
        assert max(W.nbytes(a), W.nbytes(b)) > CAP and max(len(a), len(b)) <= CAP and min(len(a), len(b)) >= 1 and W.in_bmp(a + b)
        assert max(W.nbytes(a), W.nbytes(b)) <= 4 * CAP
    assert any(max(len(a), len(b)) == CAP for a, b in rows)  # exactly at the cap
    # more than 1 024 values on one side: left to k_huge_pairs by every measure
    rows = _rows("beyond_the_cap")
    assert all(max(len(a), len(b)) > CAP for a, b in rows)
    assert any(max(len(a), len(b)) == CAP + 1 and (a + b).isascii() for a, b in rows)
    assert any(not (a + b).isascii() for a, b in rows) and any(a == "" or b == "" for a, b in rows)


def test_one_pool_forces_a_flush_on_the_job_count_and_a_first_fit_skip():
    f = W.frame()
    r = f.classes["one_pool"]
    assert r.start % W.CHUNK == 0 and len(r) == W.CHUNK  # one chunk of the work list: one pool at this frame's size
    rows = _rows("one_pool")
    assert all(a.isascii() and b.isascii() for a, b in rows)
    assert sum(max(len(a), len(b)) > 128 for a, b in rows) >= 17
    assert sum(min(len(a), len(b)) == 1024 for a, b in rows) >= 5
    batches, skips, why = W.deal(rows)
    assert sorted(i for b in batches for i in b) == list(range(W.CHUNK))
    assert "jobs" in why and "lanes" in why and skips >= 1
    assert all(len(b) <= W.LEV_JOBS for b in batches)
    assert all(sum((min(len(rows[i][0]), len(rows[i][1])) + 63) // 64 for i in b) <= 64 for b in batches)


def test_deal_restates_the_rule_on_small_cases():
    one = ("a" * 1024, "b" * 1024)
    # four 16-lane rows fill the lanes exactly: flushed on the lanes, nothing skipped
    assert W.deal([one] * 4) == ([[0, 1, 2, 3]], 0, ["lanes"])
    # five: the fifth starts a batch of its own
    assert W.deal([one] * 5)[0] == [[0, 1, 2, 3], [4]]
    # 13-lane rows: four fit (52 lanes), the fifth is passed over until the pass ends
    batches, skips, why = W.deal([("a" * 800, "b" * 1000)] * 5)
    assert batches == [[0, 1, 2, 3], [4]] and skips == 1 and why == ["pass", "pass"]
    # seventeen one-lane rows: the job list is full at sixteen
    assert W.deal([("a", "b" * 200)] * 17)[::2] == ([list(range(16)), [16]], ["jobs", "pass"])
    # the longest row ranks first; equal keys keep the order of the pool
    assert W.deal([("a", "b" * 130), ("a" * 64, "b" * 500), ("c", "d" * 130)])[0] == [[1, 0, 2]]
    # 1 024-byte texts take 1 120 bytes of the 8 192-byte arena each: the eighth does not fit
    assert W.deal([("a", "b" * 1024)] * 8)[::2] == ([list(range(7)), [7]], ["arena", "pass"])
