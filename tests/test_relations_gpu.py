"""Every measure by relations that force a pair across kernel tiers: a second opinion that needs no model.  The relations
(tests/relation_checks.py over tests/relations.py) hold on the oracle and the models (tests/test_relations_cpu.py); here they run
through strsim_amd.Context, the base pairs in the one-pair-per-lane tiers and their images beyond them, and the two must agree bit
for bit and integer for integer.  No tolerances.

Every case asserts that the crossing happened (check_tiers): by the context's counters where a call has one, else by the image's byte
lengths and ASCII-ness against the cap named in the source.
"""
import numpy as np
import pytest

import relation_checks as RC
import relation_frames as F
import relations as T

pytestmark = pytest.mark.gpu

# The lane tiers' caps, as polars-strsim_amd/csrc names them.  A pair is lane class when both strings are ASCII and at most this long.
LANE_STAGE_MAX_BYTES = 32     # k_lane_stage (strsim_lane_stage.h: "strings <= 32 ASCII bytes"): the classic five
OSA_LANE_MAX_BYTES = 64       # strsim_osa.h; also the Levenshtein / OSA distances (strsim_distance.h: dist_lane_fits)
INDEL_LANE_MAX_BYTES = 128    # strsim_indel.h: the Indel similarity and distance
PARTIAL_LANE_MAX_BYTES = 32   # strsim_partial.h: partial_ratio and its alignment
TOKEN_LANE_MAX_BYTES = 64     # strsim_token.h: a string of the token measures and of token_sort ...
TOKEN_LANE_MAX_TOKENS = 16    # ... which also holds at most this many tokens
NEAREST_MAX_LEN = 32          # strsim_nearest.h: the lane class of the three searches, queries and candidates alike
WAVE_CAP = 1024               # strsim_kernels.h: beyond it a classic measure's row waits for the long-string pass

PAIR_CAP = {"osa": OSA_LANE_MAX_BYTES, "indel": INDEL_LANE_MAX_BYTES, "partial_ratio": PARTIAL_LANE_MAX_BYTES}
PAIR_CAP.update({m: LANE_STAGE_MAX_BYTES for m in RC.CLASSIC})
DIST_CAP = {"levenshtein": OSA_LANE_MAX_BYTES, "osa": OSA_LANE_MAX_BYTES, "indel": INDEL_LANE_MAX_BYTES}


def blen(s):
    return len(s.encode("utf-8"))


def lane_string(s, cap):
    return s.isascii() and len(s) <= cap


def lane_token_string(s):
    return lane_string(s, TOKEN_LANE_MAX_BYTES) and len(s.split()) <= TOKEN_LANE_MAX_TOKENS


@pytest.fixture(scope="module")
def be():
    import strsim_amd
    with strsim_amd.Context(0) as ctx:
        yield RC.GpuBackend(ctx)


@pytest.fixture(autouse=True)
def _fresh_log(be):
    be.log.clear()  # (a test that failed before its check_tiers() leaves its calls behind)


def check_tiers(be):
    """Every call the relation filed under a role: `beyond` = rows (searches, token_sort_ratio, token_sort: strings) outside the lane
    class by construction; base and edge calls have none, image calls (nearly) all -- a pair of two empty strings stays ASCII -- and
    mixed calls some.  Where the call has a counter it must say the same."""
    seen = set()
    for e in be.log:
        role, entry, m = e["role"], e["entry"], e["measure"]
        if role is None:
            continue
        A, B = RC.bcast(e["A"], e["B"]) if entry in ("sim", "dist", "partial") else (e["A"], e["B"])
        counter = None
        if entry == "sim" and m in RC.TOKEN:
            if m == "token_sort_ratio":
                beyond, total = sum(not lane_token_string(s) for s in A + B), 2 * len(A)
            else:
                beyond, total = sum(not (lane_token_string(a) and lane_token_string(b)) for a, b in zip(A, B)), len(A)
            counter = e["token_wave"]
        elif entry == "token_sort":
            beyond, total, counter = sum(not lane_token_string(s) for s in A), len(A), e["token_wave"]
        elif entry in ("nearest", "extract", "best_match"):
            beyond, total = sum(not lane_string(s, NEAREST_MAX_LEN) for s in A + B), len(A) + len(B)
        else:
            cap = DIST_CAP[m] if entry == "dist" else PAIR_CAP[m]
            beyond, total = sum(not (lane_string(a, cap) and lane_string(b, cap)) for a, b in zip(A, B)), len(A)
            if entry == "sim" and m not in RC.CLASSIC:
                counter = e["wave"]  # (k_dist_lane / k_indel_lane / k_partial_lane count exactly the rows they leave)
        what = (role, entry, m, beyond, total, counter, e["wave"], e["late"], e["long"])
        if role in ("base", "edge"):
            assert beyond == 0, what
            if entry == "sim":  # (the calls that are retired through the context's ring: the others leave these two alone)
                assert e["late"] == 0 and e["long"] == 0, what
            if entry == "sim" and m in RC.CLASSIC:
                assert e["wave"] <= 64, what  # (only rows whose 32-byte window crosses the end of the buffer)
        elif role == "image":
            assert beyond >= 0.9 * total, what
        else:
            assert 0.05 * total <= beyond <= 0.95 * total, what
        if counter is not None:
            assert counter == beyond, what
        if entry == "sim" and m in RC.CLASSIC and role == "image":
            # (short BMP strings are decoded per lane by k_lane_utf8 and have no counter; 4-byte characters and long rows take a wave)
            if any(ord(c) > 0xFFFF for s in A[:50] + B[:50] for c in s) or min(max(blen(a), blen(b)) for a, b in zip(A, B)) > 128:
                assert e["wave"] >= 0.9 * total, what
        seen.add(role)
    be.log.clear()
    return seen


frame_of = F.frame_of


# ---- relabel ----

@pytest.mark.parametrize("base", T.RELABEL_BASES)
@pytest.mark.parametrize("m", RC.SIMILARITIES)
def test_relabel_similarity(be, m, base):
    RC.relabel_sim(be, m, base, *frame_of(m))
    assert check_tiers(be) == {"base", "image"}


@pytest.mark.parametrize("base", T.RELABEL_BASES)
@pytest.mark.parametrize("m", RC.DISTANCES)
def test_relabel_distance(be, m, base):
    RC.relabel_dist(be, m, base, *F.pair_frame())
    assert check_tiers(be) == {"base", "image"}


@pytest.mark.parametrize("base", T.RELABEL_BASES)
def test_relabel_partial_alignment(be, base):
    RC.relabel_partial(be, base, *F.pair_frame())
    assert check_tiers(be) == {"base", "image"}


@pytest.mark.parametrize("base", T.RELABEL_BASES)
def test_relabel_token_sort(be, base):
    A, B = F.token_frame()
    RC.relabel_token_sort(be, base, A + B)
    assert check_tiers(be) == {"base", "image"}
    RC.relabel_token_sort(be, base, F.token_images("unicode", "a")[0] + F.token_images("spread", "b")[1])
    be.log.clear()


# ---- common affix ----

@pytest.mark.parametrize("m,cap", [(m, cap) for m, caps in T.AFFIX_CAPS.items() for cap in caps])
def test_common_affix_distance(be, m, cap):
    n = F.N_LONG if cap >= WAVE_CAP else F.N
    A, B = F.pair_frame()
    for longest in (cap, cap + 1):
        role = "edge" if longest <= DIST_CAP[m] else "image"
        RC.affix_dist(be, m, A[:n], B[:n], *F.padded_frame(longest, n), what=f"padded to {longest} bytes", role=role)
        assert role in check_tiers(be)


@pytest.mark.parametrize("m", RC.DISTANCES)
def test_non_ascii_prefix_distance(be, m):
    A, B = F.pair_frame()
    RC.affix_dist(be, m, A, B, ["é" + a for a in A], ["é" + b for b in B], what="behind a non-ASCII prefix")
    assert check_tiers(be) == {"base", "image"}


# ---- reversal, swap, order ----

@pytest.mark.parametrize("kind,m", [("dist", m) for m in RC.DISTANCES] + [("sim", m) for m in RC.REVERSAL_SIMS])
def test_reversal(be, kind, m):
    A, B = F.pair_frame()
    A2, B2 = F.padded_frame(129, 600)  # (beyond every measure's lane tier as well)
    A3, B3 = [T.relabel(s, 0x4E00) for s in A[:600]], [T.relabel(s, 0x4E00) for s in B[:600]]
    RC.reversal(be, kind, m, A + A2 + A3, B + B2 + B3)


@pytest.mark.parametrize("kind,m", [("dist", m) for m in RC.DISTANCES] + [("sim", m) for m in RC.SWAP_SIMS])
def test_swap(be, kind, m):
    A, B = frame_of(m)
    A2, B2 = F.padded_frame(129, 600)
    A3, B3 = [T.relabel(s, 0x400) for s in A[:600]], [T.relabel(s, 0x400) for s in B[:600]]
    RC.swap(be, kind, m, A + A2 + A3, B + B2 + B3)


@pytest.mark.parametrize("image", ["base", "relabelled", "padded to 65", "padded to 129"])
def test_distance_order(be, image):
    A, B = F.pair_frame()
    if image == "relabelled":
        A, B = [T.relabel(s, 0x1F600) for s in A], [T.relabel(s, 0x1F600) for s in B]
    elif image != "base":
        A, B = F.padded_frame(int(image.split()[-1]), F.N)
    lev, osa, ind = RC.distance_order(be, A, B)
    assert (osa < lev).mean() > 0.02 and (lev < ind).mean() > 0.3


# ---- partial ratio ----

def test_partial_alignment_spans_score_as_indel(be):
    A, B = F.pair_frame()
    assert RC.partial_spans_are_indel(be, A, B) > 0.9 * F.N
    RC.partial_spans_are_indel(be, [T.relabel(s, 0x400) for s in A], [T.relabel(s, 0x400) for s in B])
    RC.partial_spans_are_indel(be, *F.padded_frame(33, F.N))


def test_partial_ratio_of_a_contained_needle(be):
    RC.partial_contained(be, *F.contained_frame())
    assert check_tiers(be) == {"mixed"}


def test_partial_ratio_at_least_indel_for_equal_lengths(be):
    A, B = F.equal_length_frame()
    RC.partial_at_least_indel(be, A, B)
    RC.partial_at_least_indel(be, [T.relabel(s, 0x4E00) for s in A], [T.relabel(s, 0x4E00) for s in B])
    RC.partial_at_least_indel(be, ["xyz" + a for a in A], ["xyz" + b for b in B])  # (31 .. 33 bytes among them)


# ---- token measures ----

@pytest.mark.parametrize("m,mode", [(m, mode) for m in RC.TOKEN for mode in ("spread", "unicode")] + [("token_set_ratio", "copies")])
def test_token_invariance(be, m, mode):
    A, B = F.token_frame()
    for side in ("a", "b"):
        RC.token_invariance(be, m, A, B, *F.token_images(mode, side), what=f"with side {side} permuted ({mode})",
                            role="image" if mode != "copies" and m == "token_set_ratio" else "mixed")  # (token_sort_ratio counts strings: one side)
        assert "base" in check_tiers(be)


def test_token_sort_is_idempotent(be):
    A, B = F.token_frame()
    A2, B2 = F.token_images("unicode", "a")[0], F.token_images("spread", "b")[1]
    once = RC.token_sort_idempotent(be, A + B, role="base")
    assert once == [" ".join(sorted(s.split())) for s in A + B]
    RC.token_sort_idempotent(be, B2, role="image")
    RC.token_sort_idempotent(be, A + A2 + B2, role="mixed")
    assert check_tiers(be) == {"base", "image", "mixed"}


def test_token_sort_ratio_is_indel_of_the_sorted_strings(be):
    A, B = F.token_frame()
    RC.token_sort_ratio_is_indel(be, A, B, role="base")
    RC.token_sort_ratio_is_indel(be, F.token_images("unicode", "a")[0], F.token_images("spread", "b")[1], role="image")
    assert check_tiers(be) == {"base", "image"}


# ---- batch level ----

KINDS = [("sim", m) for m in RC.SIMILARITIES] + [("dist", m) for m in RC.DISTANCES]


mixed_frame = F.mixed_frame


def cutoff_of(kind, m):
    return RC.CUTOFFS[m][1] if kind == "dist" else None


@pytest.mark.parametrize("kind,m", KINDS)
def test_batch_row_permutation(be, kind, m):
    """The lane kernels sort and deal rows in 512-row blocks: a row's neighbours change its round, never its value."""
    X, Y = mixed_frame(m)
    RC.batch_permutation(be, kind, m, X, Y, cutoff_of(kind, m), 9)
    RC.batch_permutation(be, kind, m, *frame_of(m), cutoff_of(kind, m), 10)


@pytest.mark.parametrize("kind,m", KINDS)
def test_batch_concatenation(be, kind, m):
    A, B = frame_of(m)
    X, Y = mixed_frame(m)
    RC.batch_concatenation(be, kind, m, A[:1500], B[:1500], X[1500:], Y[1500:], cutoff_of(kind, m))
    if kind == "sim" and m in RC.CLASSIC:  # (the frame's 40 rows beyond WAVE_CAP went to the long-string pass)
        assert [e["long"] for e in be.log if e["role"] == "mixed"] == [40]
    assert check_tiers(be) == {"base", "mixed"}


@pytest.mark.parametrize("kind,m", KINDS)
def test_batch_literal(be, kind, m):
    A, B = frame_of(m)
    X, _ = mixed_frame(m)
    for lit in (B[7], T.relabel(B[8], 0x4E00), "ab " * 30):
        assert lit
        RC.batch_literal(be, kind, m, X[:2600], lit, cutoff_of(kind, m))
    RC.batch_literal(be, kind, m, A[:1000], "", cutoff_of(kind, m))


@pytest.mark.parametrize("kind,m", KINDS)
def test_batch_host_against_device(be, kind, m):
    import torch
    X, Y = mixed_frame(m)
    S, ctx = be.S, be.ctx
    cols = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:%d" % ctx.device) for x in S.pack_strings(X) + S.pack_strings(Y)]
    k = cutoff_of(kind, m)
    if kind == "sim":
        out = ctx.pairs_device(m, *cols)
    else:
        out = ctx.distance_device(m, *cols, k)
    torch.cuda.synchronize()
    ctx.synchronize()
    got = out.cpu().numpy()
    RC.same(kind, got if kind == "sim" else got.view(np.uint32), RC.call(be, kind, m, X, Y, k), X, Y, f"{m} {kind}: device call against host call")


# ---- searches ----

def _relabelled(X, base):
    return [T.relabel(s, base) for s in X]


@pytest.mark.parametrize("image", ["relabelled 2 bytes", "relabelled 4 bytes", "prefixed"])
@pytest.mark.parametrize("m", ("levenshtein", "osa"))
def test_search_nearest(be, m, image):
    Q, Cs = F.search_frame()
    if image == "prefixed":
        Q2, Cs2 = [F.SEARCH_PREFIX + s for s in Q], [F.SEARCH_PREFIX + s for s in Cs]
        assert all(s.isascii() and len(s) > NEAREST_MAX_LEN for s in Q2 + Cs2)
    else:
        base = 0x400 if "2" in image else 0x1F600
        Q2, Cs2 = _relabelled(Q, base), _relabelled(Cs, base)
    for k in F.SEARCH_KS:
        for md in (F.NEAREST_CUTOFF, None):
            RC.search_invariance(be, "nearest", m, Q, Cs, Q2, Cs2, k, md, image)
    assert check_tiers(be) == {"base", "image"}


@pytest.mark.parametrize("base", T.RELABEL_BASES)
@pytest.mark.parametrize("scorer", ("indel", "token_sort_ratio"))
def test_search_extract(be, scorer, base):
    Q, Cs = F.token_search_frame() if scorer == "token_sort_ratio" else F.search_frame()
    for k in F.SEARCH_KS:
        for cut in (F.EXTRACT_CUTOFF[scorer], None):
            RC.search_invariance(be, "extract", scorer, Q, Cs, _relabelled(Q, base), _relabelled(Cs, base), k, cut, "relabelled")
    assert check_tiers(be) == {"base", "image"}


@pytest.mark.parametrize("base", (0x400, 0x1F600))
@pytest.mark.parametrize("m", RC.CLASSIC)
def test_search_best_match(be, m, base):
    Q, Cs = F.search_frame()
    for k in F.SEARCH_KS:
        for cut in (F.BEST_MATCH_CUTOFF[m], None):
            RC.search_invariance(be, "best_match", m, Q, Cs, _relabelled(Q, base), _relabelled(Cs, base), k, cut, "relabelled")
    assert check_tiers(be) == {"base", "image"}
