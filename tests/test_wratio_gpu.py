"""token_ratio, partial_token_sort_ratio, partial_token_set_ratio, partial_token_ratio and wratio (ids 18 .. 26) on the GPU, bit
for bit against tests/wratio_ref.py: the main frame of tests/wratio_frames.py through strsim_pairs_device, the relations between
the measures computed on the GPU, how wratio routes its rows, every row count around the wave, the gather's scan block and its
lane groups, literals, the host entry point on both of its paths, the small-call entry point, and calls back to back on one
context."""
import numpy as np
import pytest

import wratio_frames as F
import wratio_ref as W

pytestmark = pytest.mark.gpu

NAMES = ("token_ratio", "partial_token_sort_ratio", "partial_token_set_ratio", "partial_token_ratio", "wratio")


@pytest.fixture(scope="module")
def S():
    import strsim_amd
    return strsim_amd


@pytest.fixture(scope="module")
def ctx(S):
    with S.Context(0) as c:
        yield c


def same_bits(got, exp, what=""):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, what
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, (what, [(int(i), float(got[i]), float(exp[i])) for i in bad[:8]])


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def device_columns(S, A, B):
    return tuple(dev(x) for x in S.pack_strings(A)) + tuple(dev(x) for x in S.pack_strings(B))


def on_device(S, c, measure, A, B):
    """strsim_pairs_device over device-resident columns -> numpy (a frame without rows has no device column: the host call)"""
    if len(A) == 0 or len(B) == 0:
        return on_host(S, c, measure, A, B)
    ao, av, bo, bv = device_columns(S, A, B)
    out = c.pairs_device(measure, ao, av, bo, bv)
    c.synchronize()
    return out.cpu().numpy()


def on_host(S, c, measure, A, B):
    ao, av = S.pack_strings(A)
    bo, bv = S.pack_strings(B)
    return c.pairs_host(measure, ao, av, bo, bv)


def counts(cls):
    return int((cls == W.NEAR).sum()), int((cls >= W.FAR8).sum())


# ---- the main frame ----

@pytest.mark.parametrize("name", NAMES)
def test_wratio_main_frame_on_the_device(S, ctx, name):
    A, B, cols = F.main()
    assert 6000 <= len(A) <= 8000
    same_bits(on_device(S, ctx, name, A, B), cols[name], name)
    if name == "wratio":
        assert ctx.last_wratio_rows() == counts(cols["class"])
        near, far = counts(cols["class"])
        assert near > 4096 and far > 2000 and near + far < len(A)  # (every class is there)


def test_wratio_known_answers_and_nulls(S, ctx):
    A = ["this is a test", "fuzzy wuzzy was a bear", "ab ab", "", " ", None, "éé"]
    B = ["this is a new test!!!", "wuzzy fuzzy was a bear", "abab", "", "\t", "x", None]
    got = S.wratio(A, B, ctx=ctx)
    assert got[0] == (1.0 * 0.95) * 0.9 and got[1] == 0.95 and got[3] == 0.0 and got[4] == 0.95
    assert np.isnan(got[5]) and np.isnan(got[6])
    assert S.token_ratio(A[:3], B[:3], ctx=ctx).tolist()[1] == 1.0
    assert S.partial_token_sort_ratio(A[:3], B[:3], ctx=ctx).tolist()[1:] == [1.0, 0.75]
    assert S.partial_token_set_ratio(A[:3], B[:3], ctx=ctx).tolist() == [1.0, 1.0, 1.0]
    assert S.partial_token_ratio(A[:3], B[:3], ctx=ctx).tolist() == [1.0, 1.0, 1.0]
    for name in NAMES:  # both argument orders against the model, row by row
        exp = [W.SCORE[name](a, b) for a, b in zip(A[:5], B[:5])]
        same_bits(S.similarity(name, A[:5], B[:5], ctx=ctx), exp, name)
        same_bits(S.similarity(name, B[:5], A[:5], ctx=ctx), [W.SCORE[name](b, a) for a, b in zip(A[:5], B[:5])], name)


# ---- relations, computed on the GPU ----

def test_wratio_relations_between_the_gpu_columns(S, ctx):
    A, B, cols = F.main()
    g = {m: on_device(S, ctx, m, A, B) for m in ("indel", "partial_ratio", "token_sort_ratio", "token_set_ratio") + NAMES}
    same_bits(g["token_ratio"], np.maximum(g["token_sort_ratio"], g["token_set_ratio"]), "token_ratio == max(sort, set)")
    SA, SB = S.token_sort(A, ctx=ctx), S.token_sort(B, ctx=ctx)
    same_bits(g["partial_token_sort_ratio"], on_device(S, ctx, "partial_ratio", SA, SB), "partial_ratio of the token_sort columns")
    same_bits(g["partial_token_ratio"], np.maximum(g["partial_token_sort_ratio"], g["partial_token_set_ratio"]), "max of the partial forms")
    cls = np.array([W.wratio_class(len(a), len(b)) for a, b in zip(A, B)], dtype=np.uint8)
    host = W.combine(cls, g["indel"], np.maximum(g["token_sort_ratio"], g["token_set_ratio"]), g["partial_ratio"],
                     np.maximum(g["partial_token_sort_ratio"], g["partial_token_set_ratio"]))
    same_bits(g["wratio"], host, "the combine rule over the six GPU columns")


# ---- routing ----

def test_wratio_routing_all_near_all_far_all_empty(S):
    near_idx, far_idx = F.rows_of_class(W.NEAR)[:600], F.rows_of_class(W.FAR8, W.FAR)[:600]
    # rows no kernel leaves to a one-pair-per-wave tier: the launches of a call depend on its routing alone
    A, B, _ = F.main()
    short = lambda i: A[i].isascii() and B[i].isascii() and len(A[i]) <= 30 and len(B[i]) <= 30  # noqa: E731
    near_idx = np.array([i for i in near_idx if short(i)])
    far_idx = np.array([i for i in far_idx if short(i)])
    assert near_idx.size > 300 and far_idx.size > 300
    ops = {}
    with S.Context(0) as c:
        def run(key, A2, B2, exp, want):
            before = c.enqueued_ops
            same_bits(on_device(S, c, "wratio", A2, B2), exp, key)
            ops[key] = c.enqueued_ops - before
            assert c.last_wratio_rows() == want, key
            assert c.last_token_wave_rows == 0 and c.last_late_rows == 0, key

        An, Bn, cn = F.take(near_idx)
        Af, Bf, cf = F.take(far_idx)
        run("near", An, Bn, cn["wratio"], (len(An), 0))
        run("far", Af, Bf, cf["wratio"], (0, len(Af)))
        run("empty", [""] * 100 + ["abc"] * 30, ["x y"] * 100 + [""] * 30, np.zeros(130), (0, 0))
        run("near+1", An + Af[:1], Bn + Bf[:1], np.concatenate([cn["wratio"], cf["wratio"][:1]]), (len(An), 1))
        run("far+1", Af + An[:1], Bf + Bn[:1], np.concatenate([cf["wratio"], cn["wratio"][:1]]), (1, len(Af)))
        run("far, fewer rows", Af[:77], Bf[:77], cf["wratio"][:77], (0, 77))
    # A family without rows launches nothing: one row of the other class adds that family's launches, and the two mixed frames
    # launch the same; the all-empty frame launches neither family.
    assert ops["empty"] < ops["near"] < ops["near+1"] and ops["empty"] < ops["far"] < ops["far+1"]
    assert ops["near+1"] == ops["far+1"] and ops["far, fewer rows"] == ops["far"]
    assert ops["near+1"] - ops["empty"] == (ops["near"] - ops["empty"]) + (ops["far"] - ops["empty"])


# ---- row counts ----

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4096, 4097])
def test_wratio_row_counts(S, ctx, n):
    """A mixed frame of n rows, and n near rows: at 4 097 the near list is longer than one block of the gather's scan."""
    for idx in (F.mixed(n), F.rows_of_class(W.NEAR)[:n]):
        assert len(idx) == n
        A, B, cols = F.take(idx)
        for name in NAMES if n <= 257 else ("wratio",):
            same_bits(on_device(S, ctx, name, A, B), cols[name], (name, n))
        if n:  # (a call without rows returns before it routes anything)
            assert ctx.last_wratio_rows() == counts(cols["class"])
    far = F.rows_of_class(W.FAR8, W.FAR)[:min(n, 300)]
    A, B, cols = F.take(far)
    same_bits(on_device(S, ctx, "wratio", A, B), cols["wratio"], ("far", n))


# ---- call forms ----

def test_wratio_literal_on_either_side(S, ctx):
    A, B, _ = F.take(F.mixed(300, seed=11))
    A += ["", "   ", "日本 ab"]
    fr = F.frames()
    for lit in ("ab cd", "é", "", "ab  ab cab abc b ba xyz"):
        for X, Y in ((A, [lit]), ([lit], A)):
            cols = fr.columns(X, Y)
            for name in NAMES:
                same_bits(on_device(S, ctx, name, X, Y), cols[name], (name, lit, len(X)))
            assert ctx.last_wratio_rows() == counts(cols["class"])
    cols = fr.columns(["ab cd"], ["cd ab x"])
    for name in NAMES:  # a literal against a literal: one row
        same_bits(on_device(S, ctx, name, ["ab cd"], ["cd ab x"]), cols[name], name)


def test_wratio_host_entry_point_on_both_paths(S, monkeypatch):
    """strsim_pairs_host computes small calls in place on pinned memory and stages large ones: both against the model."""
    A, B, cols = F.take(F.mixed(700, seed=3))
    for direct in ("0", None):
        if direct is not None:
            monkeypatch.setenv("STRSIM_HOST_DIRECT_ROWS", direct)
        else:
            monkeypatch.delenv("STRSIM_HOST_DIRECT_ROWS", raising=False)
        with S.Context(0) as c:
            for name in NAMES:
                same_bits(on_host(S, c, name, A, B), cols[name], (name, direct))
            assert c.last_wratio_rows() == counts(cols["class"])
            assert on_host(S, c, "wratio", [], []).size == 0


def test_wratio_small_call_entry_point(S):
    A, B, cols = F.take(F.mixed(100, seed=5))
    import torch
    with S.Context(0) as c:
        ao, av, bo, bv = device_columns(S, A, B)
        for name in NAMES:
            out = torch.empty(len(A), dtype=torch.float64, device="cuda:0")
            rc = S.lib().strsim_pairs_device_small(c._h, S.MEASURE_ID[name], ao.data_ptr(), av.data_ptr(), len(A), bo.data_ptr(), bv.data_ptr(),
                                                   len(B), out.data_ptr(), len(A))
            assert rc == 0, S.lib().strsim_last_error_message()
            c.synchronize()
            same_bits(out.cpu().numpy(), cols[name], name)


def test_wratio_calls_back_to_back_on_one_context(S):
    """Two wratio calls and an indel call enqueued without a wait between them: the scratch of one call is not the next one's."""
    A1, B1, c1 = F.take(F.mixed(3000, seed=1))
    A2, B2, c2 = F.take(F.mixed(500, seed=2))
    with S.Context(0) as c:
        d1, d2 = device_columns(S, A1, B1), device_columns(S, A2, B2)
        o1 = c.pairs_device("wratio", *d1)
        o2 = c.pairs_device("wratio", *d2)
        o3 = c.pairs_device("indel", *d1)
        o4 = c.pairs_device("partial_token_ratio", *d2)
        o5 = c.pairs_device("token_ratio", *d1)
        c.synchronize()
        same_bits(o1.cpu().numpy(), c1["wratio"], "first")
        same_bits(o2.cpu().numpy(), c2["wratio"], "second")
        same_bits(o3.cpu().numpy(), c1["indel"], "indel")
        same_bits(o4.cpu().numpy(), c2["partial_token_ratio"], "partial_token_ratio")
        same_bits(o5.cpu().numpy(), c1["token_ratio"], "token_ratio")
        assert c.last_wratio_rows() == counts(c2["class"])


def test_wratio_shape_errors_on_the_device(S, ctx):
    with pytest.raises(S.ShapeMismatch):
        S.wratio(["a", "b"], ["a", "b", "c"], ctx=ctx)
    assert S.wratio([], [], ctx=ctx).size == 0
