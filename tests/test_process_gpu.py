"""default_process and processed scoring on the GPU: the transform byte for byte (offsets and values) against tests/process_ref.py
on the frame of tests/process_frames.py, row counts around the wave and block sizes, a non-zero offsets base, the capacity rule,
idempotence on the device, the wave-tier counter, calls back to back; processed scoring bit for bit against the pairwise call over
the transformed columns and against each measure's model over the model's processed strings; extract with a processor."""
import numpy as np
import pytest

import indel_ref
import model_py
import process_frames as F
import process_ref as R
import token_ref
import wratio_ref

pytestmark = pytest.mark.gpu

MEASURES = ("indel", "levenshtein", "jaro_winkler", "partial_ratio", "token_set_ratio", "wratio")
MODEL = {"indel": indel_ref.score, "levenshtein": model_py.levenshtein, "jaro_winkler": model_py.jaro_winkler,
         "partial_ratio": wratio_ref.partial_ratio, "token_set_ratio": token_ref.set_rule, "wratio": wratio_ref.wratio}


@pytest.fixture(scope="module")
def S():
    import strsim_amd
    return strsim_amd


@pytest.fixture(scope="module")
def ctx(S):
    with S.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def same_bits(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, [(int(i), float(got[i]), float(exp[i])) for i in bad[:8]]


def check_column(S, ctx, rows, want=None):
    """The host call over `rows` against the model: offsets and values, byte for byte; returns the wave-tier count."""
    want = [R.default_process(s) for s in rows] if want is None else list(want)
    off, val = ctx.default_process_host(*S.pack_strings(list(rows)))
    eo, ev = S.pack_strings(want)
    assert off.dtype == np.uint32 and off.shape == eo.shape
    bad = np.flatnonzero(off != eo)
    assert bad.size == 0, [(int(i), rows[max(int(i) - 1, 0)]) for i in bad[:4]]
    assert val.tobytes() == ev.tobytes()
    return ctx.last_process_wave_rows


def to_device(torch, S, rows, base=0, front=b""):
    """A device column whose offsets start at `base` (the values carry `front`, base bytes that belong to no row)."""
    off, val = S.pack_strings(list(rows))
    assert len(front) == base
    val = np.concatenate([np.frombuffer(front, dtype=np.uint8), val])
    d_off = torch.from_numpy((off.astype(np.int64) + base).astype(np.int32)).cuda()
    d_val = torch.from_numpy(np.concatenate([val, np.zeros(1, dtype=np.uint8)])).cuda()
    return d_off, d_val


def from_device(off, val):
    off = off.cpu().numpy().astype(np.uint32)
    raw = val.cpu().numpy().tobytes()
    return [raw[int(off[i]):int(off[i + 1])].decode("utf-8") for i in range(off.size - 1)], off


def test_frame_byte_for_byte(S, ctx):
    rows, want = F.frame(), F.expected()
    assert 2800 <= len(rows) <= 3300
    assert any(len(w.encode()) > len(r.encode()) for r, w in zip(rows, want))      # a row that grows
    assert sum(w == "" for w in want) > 50 and max(len(r.encode()) for r in rows) > 5000
    waves = check_column(S, ctx, rows, want)
    assert waves == sum(not F.is_lane_row(s) for s in rows)
    assert S.default_process(list(rows[:200]) + [None], ctx=ctx) == list(want[:200]) + [None]


def test_known_answers(S, ctx):
    got = S.default_process(["Apple, Inc.", "apple inc", "Ⱥ_Kİ\U00010400\U0001D11Eẞ9\x00", "!!!", "ÀÉ　x", None, "", "ΑΣ", "İ"],
                            ctx=ctx)
    assert got == ["apple  inc", "apple inc", "ⱥ_ki\U00010428 ß9", "", "àé x", None, "", "ασ", "i"]
    a, b = ["Apple, Inc."], ["apple inc"]
    assert S.indel(a, b, ctx=ctx)[0] == 0.7 and S.token_sort_ratio(a, b, ctx=ctx)[0] == 0.7
    assert S.indel(a, b, ctx=ctx, processor="default_process")[0] == 1 - 1 / 19 == 0.9473684210526316
    assert S.token_sort_ratio(a, b, ctx=ctx, processor="default_process")[0] == 1.0
    assert np.isnan(S.indel(["x", None], ["x", "y"], ctx=ctx, processor="default_process")[1])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_row_counts(S, ctx, n):
    rows = F.frame()
    rows = [rows[i % len(rows)] for i in range(n)]
    check_column(S, ctx, rows)


def test_lane_limit(S, ctx):
    """limit - 1, limit and limit + 1 bytes of ASCII: the last two lengths of the lane tier and the first of the wave tier."""
    L = F.LANE_MAX_BYTES
    rows = [(" ,Ab_" * 20)[:n] for n in (L - 1, L, L + 1)] + ["x" * (L - 1), "Y" * L, "z" * (L + 1), "." * L, "." * (L + 1)]
    assert check_column(S, ctx, rows) == 3
    assert check_column(S, ctx, rows[:2] + rows[3:5] + rows[6:7]) == 0


def test_offsets_base_and_device_call(S, ctx, torch):
    rows = list(F.frame()[:500])
    front = b"Q\xc8\xbaz, "   # bytes in front of the first row: letters and half a sentence that belong to no row
    d_off, d_val = to_device(torch, S, rows, base=len(front), front=front)
    o_off, o_val = ctx.default_process_device(d_off, d_val)
    ctx.synchronize()
    got, off = from_device(o_off, o_val)
    assert off[0] == 0 and got == [R.default_process(s) for s in rows]


def test_capacity(S, ctx, torch):
    rows = ["Ⱥ" * 10, "Ⱦ", "ȺȾȺ"]             # only growers: 28 bytes become 42
    d_off, d_val = to_device(torch, S, rows)
    total = 42
    out_off = torch.empty(len(rows) + 1, dtype=torch.int32, device="cuda")
    guard = torch.full((total + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(S.StrsimError, match=r"out_capacity=41 but the processed column holds 42 bytes"):
        ctx.default_process_device(d_off, d_val, out_off, guard[:total - 1])
    ctx.synchronize()
    assert bool((guard == 0xA5).all())          # a refused call writes no value
    ctx.default_process_device(d_off, d_val, out_off, guard[:total])
    ctx.synchronize()
    got, off = from_device(out_off, guard[:total])
    assert got == [R.default_process(s) for s in rows] and int(off[-1]) == total == 28 + 28 // 2
    assert bool((guard[total:] == 0xA5).all())  # ... and an accepted one nothing behind the exact size


def test_idempotent_on_the_device(S, ctx, torch):
    d_off, d_val = to_device(torch, S, F.frame())
    o1, v1 = ctx.default_process_device(d_off, d_val)
    o2, v2 = ctx.default_process_device(o1, v1)
    ctx.synchronize()
    n = int(o1[-1])
    assert torch.equal(o1, o2) and torch.equal(v1[:n], v2[:n])


def test_wave_rows_counter_and_back_to_back_calls(S, ctx, torch):
    lane_only = [s for s in F.frame() if F.is_lane_row(s)][:700]
    assert check_column(S, ctx, lane_only) == 0
    mixed = list(F.frame()[:900])
    cols = [to_device(torch, S, c) for c in (lane_only, mixed, lane_only[:65], mixed[:64])]
    outs = [ctx.default_process_device(o, v) for o, v in cols]   # four calls before anything is read
    assert ctx.last_process_wave_rows == sum(not F.is_lane_row(s) for s in mixed[:64])
    ctx.synchronize()
    for (o, v), rows in zip(outs, (lane_only, mixed, lane_only[:65], mixed[:64])):
        assert from_device(o, v)[0] == [R.default_process(s) for s in rows]


# ---- processed scoring ----

@pytest.fixture(scope="module")
def pairs(S, torch):
    A, B = F.pair_frame()
    return {"A": A, "B": B, "PA": [R.default_process(s) for s in A], "PB": [R.default_process(s) for s in B],
            "dA": to_device(torch, S, A), "dB": to_device(torch, S, B)}


@pytest.mark.parametrize("measure", MEASURES)
def test_pairs_processed(S, ctx, pairs, measure):
    A, B = pairs["A"], pairs["B"]
    got = ctx.pairs_processed_device(measure, *pairs["dA"], *pairs["dB"])
    ctx.synchronize()
    waves = ctx.last_process_wave_rows
    got = got.cpu().numpy()
    # bit for bit the pairwise call over the columns the transform writes
    pa, pb = ctx.default_process_device(*pairs["dA"]), ctx.default_process_device(*pairs["dB"])
    two_step = ctx.pairs_device(measure, *pa, *pb)
    ctx.synchronize()
    same_bits(got, two_step.cpu().numpy())
    # ... the measure's model over the model's processed strings
    same_bits(got, [MODEL[measure](a, b) for a, b in zip(pairs["PA"], pairs["PB"])])
    # ... and the host call and the Python surface
    same_bits(ctx.pairs_processed_host(measure, *S.pack_strings(list(A)), *S.pack_strings(list(B))), got)
    same_bits(S.similarity(measure, list(A), list(B), ctx=ctx, processor="default_process"), got)
    assert waves == sum(not F.is_lane_row(s) for s in A) + sum(not F.is_lane_row(s) for s in B)


@pytest.mark.parametrize("measure", MEASURES)
def test_pairs_processed_literal_on_either_side(S, ctx, pairs, measure):
    A = list(pairs["A"][:200])
    lit = "École, GMBH & co-op"
    plit = R.default_process(lit)
    for flip in (False, True):
        x, y = ([lit], A) if flip else (A, [lit])
        got = ctx.pairs_processed_host(measure, *S.pack_strings(x), *S.pack_strings(y))
        px, py = ([plit], pairs["PA"][:200]) if flip else (pairs["PA"][:200], [plit])
        same_bits(got, ctx.pairs_host(measure, *S.pack_strings(px), *S.pack_strings(py)))
        f = MODEL[measure]
        same_bits(got, [f(plit, p) if flip else f(p, plit) for p in pairs["PA"][:200]])


def test_pairs_processed_back_to_back_with_a_pending_long_row(S, ctx, torch):
    """Two processed levenshtein calls with nothing between them.  The first holds a row beyond the wave kernel's 1 024 bytes, whose
    pass runs when the call is retired and reads the call's (processed) columns again; the second processes larger columns into
    the same scratch.  The second call retires the first before it touches that scratch, so both are what they are alone."""
    long_a, long_b = "Ab, " * 300, "ab  " * 299 + "xy"       # processed: 1 198 characters each, the last two differ
    A1, B1 = ["Apple, Inc.", long_a, "x"], ["apple inc", long_b, "Y!"]
    A2, B2 = F.pair_frame()
    A2, B2 = list(A2) * 4, list(B2) * 4                        # 2 400 rows: larger offsets and values than the first call's
    d1, d2 = (to_device(torch, S, A1), to_device(torch, S, B1)), (to_device(torch, S, A2), to_device(torch, S, B2))
    out1 = ctx.pairs_processed_device("levenshtein", *d1[0], *d1[1])
    out2 = ctx.pairs_processed_device("levenshtein", *d2[0], *d2[1])
    ctx.synchronize()
    assert ctx.last_long_rows == 1                             # (retired inside the second call, reported with this synchronize)
    got1, got2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert got1[1] == 1 - 2 / 1198
    same_bits(got1[[0, 2]], [model_py.levenshtein("apple  inc", "apple inc"), model_py.levenshtein("x", "y")])
    alone = ctx.pairs_processed_device("levenshtein", *d2[0], *d2[1])
    ctx.synchronize()
    same_bits(got2, alone.cpu().numpy())
    same_bits(got2[:600], [model_py.levenshtein(R.default_process(a), R.default_process(b)) for a, b in zip(A2[:600], B2[:600])])


def test_wave_rows_counter_is_of_the_last_call(S, ctx, torch):
    ctx.default_process_device(*to_device(torch, S, ["é", "ü", "a"]))
    assert ctx.last_process_wave_rows == 2
    ctx.default_process_device(*to_device(torch, S, []))       # zero rows: the count is this call's, not the one before
    assert ctx.last_process_wave_rows == 0


def test_unknown_processor_and_measure(S, ctx, pairs):
    with pytest.raises(ValueError, match="unknown processor"):
        ctx.pairs_processed_device("indel", *pairs["dA"], *pairs["dB"], processor="lower")
    for measure in (5, 27, 28):
        with pytest.raises(S.StrsimError, match="unknown measure %d" % measure):
            ctx.pairs_processed_device(measure, *pairs["dA"], *pairs["dB"])


@pytest.mark.parametrize("scorer", ["ratio", "token_sort_ratio"])
def test_extract_with_processor(S, ctx, scorer):
    A, B = F.pair_frame()
    queries, cands = list(A[:60]) + [None, "!!!"], list(B[:90]) + [None, "", "APPLE, inc"]
    idx, score = S.extract(scorer, queries, cands, k=3, score_cutoff=0.4, ctx=ctx, processor="default_process")
    pq, pc = [R.default_process(s) for s in queries], [R.default_process(s) for s in cands]
    eidx, escore = S.extract(scorer, pq, pc, k=3, score_cutoff=0.4, ctx=ctx)
    assert np.array_equal(idx, eidx)
    same_bits(score, escore)
    assert (idx >= 0).any() and (idx[-2] == -1).all()
