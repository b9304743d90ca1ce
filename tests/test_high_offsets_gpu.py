"""Every device entry point with its columns placed anywhere in the first 4 GiB behind the values pointer (tests/high_offsets.py):
offsets whose top bit is set, a row that holds byte 2^31, columns that end at 0xFFFFFFFF, at the end of a 16-byte chunk and one byte
before it.  Every result is compared with the model the entry point's own suite uses -- f64 by its bits, integers, indices, CSR arrays
and bytes exactly -- and the same call with its columns at base 0 must give the model's values too, so a wrong expected column
cannot pass everywhere.  After every call the tier counters are compared with those of the call at base 0: a row that a byte from
outside its column sent to a slower tier has the right score and a wrong counter.

The frame of the pairwise entry points is relation_frames.mixed_frame (rows of every tier; long rows last), run as it is, with its
rows reversed (a long row first, lane-class rows last) and with an empty last row.  The models of partial_ratio and of the
measures built on it are brute forces over every window, about 1.4 s for a row of 1 025 bytes: and the wave kernel takes a third of a second for
one: their frames keep one of the frame's 40 rows of that length -- rows cut, no placement.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import gen
import high_offsets as H
import relation_checks as RC
import relation_frames as F

pytestmark = pytest.mark.gpu

LANE_STAGE_MAX_BYTES = 32  # k_lane_stage: both strings ASCII and at most this long (tests/test_relations_gpu.py)
LONG_ROWS = 40             # mixed_frame's last rows: beyond WAVE_CAP
VARIANTS = ("forward", "reversed", "empty_last")
WEIGHTED = ("token_ratio", "partial_token_sort_ratio", "partial_token_set_ratio", "partial_token_ratio", "wratio")
PAIR_MEASURES = RC.CLASSIC + RC.NEWER + RC.TOKEN + WEIGHTED
QGRAMS = (("jaccard", 2, True), ("cosine", 3, False), ("sorensen_dice", 1, True))
PAIR_IDS = ["%s-%s" % p for p in H.PAIRS]
# a second column for every placement of a first one: each column of a two-column call sees all six
PARTNER = {"low": "top1", "sign_short": "top16", "sign_long": "top17", "top1": "low", "top16": "sign_short", "top17": "sign_long"}
# the two-column calls of the matrix entry points: the pairs of H.PAIRS whose first placement is one of the three
THREE = {"sign_short": "top1", "sign_long": "sign_short", "top1": "sign_long"}
K = 3


# ---- frames and models: built once, shared, never changed ----

def cut_long(X, keep):
    return X[:len(X) - LONG_ROWS] + X[len(X) - LONG_ROWS:len(X) - LONG_ROWS + keep]


@functools.lru_cache(maxsize=None)
def frame(kind):
    """-> (A, B) as tuples, an empty row appended to both: the "empty_last" variant; the others leave it out."""
    base, _, keep = kind.partition("/")
    A, B = F.mixed_frame("token_sort_ratio" if base == "token" else "levenshtein")
    if keep:
        A, B = cut_long(A, int(keep)), cut_long(B, int(keep))
    return tuple(A) + ("",), tuple(B) + ("",)


def kind_of(m):
    if m in WEIGHTED:
        return "token/1"
    if m == "partial_ratio":
        return "pair/1"
    return "token" if m in RC.TOKEN else "pair"


def variant(X, v):
    """rows of a frame() column, or of a model's result over it"""
    if v == "empty_last":
        return X
    return X[:-1] if v == "forward" else X[:-1][::-1]


@functools.lru_cache(maxsize=None)
def models():
    return RC.ModelBackend()


@functools.lru_cache(maxsize=None)
def weighted_columns(kind, processed=False):
    import process_ref
    import wratio_ref
    A, B = frame(kind)
    if processed:
        A, B = process_ref.default_process_column(A), process_ref.default_process_column(B)
    return wratio_ref.Frames().columns(list(A), list(B))


@functools.lru_cache(maxsize=None)
def partial_model(kind):
    A, B = frame(kind)
    return models().partial(list(A), list(B))


@functools.lru_cache(maxsize=None)
def sim_model(m):
    A, B = frame(kind_of(m))
    if m in WEIGHTED:
        return weighted_columns(kind_of(m))[m]
    if m == "partial_ratio":
        return partial_model(kind_of(m))[0]
    return models().sim(m, list(A), list(B))


@functools.lru_cache(maxsize=None)
def dist_model(m, k):
    A, B = frame("pair")
    return models().dist(m, list(A), list(B), k)


@functools.lru_cache(maxsize=None)
def qgram_model(kind, q, multiset):
    import qgram_ref
    A, B = frame("pair")
    return np.array(qgram_ref.batch(kind, list(A), list(B), q, multiset), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def processed_model(m):
    import process_ref
    if m == "wratio":
        return weighted_columns("token/1", True)["wratio"]
    A, B = frame("pair")
    return models().sim(m, process_ref.default_process_column(A), process_ref.default_process_column(B))


@functools.lru_cache(maxsize=None)
def transform_model(name):
    import process_ref
    import token_ref
    X = frame("token")[0]
    return tuple(token_ref.token_sort(s) for s in X) if name == "token_sort" else tuple(process_ref.default_process_column(X))


@functools.lru_cache(maxsize=None)
def literal_model(m, lit, side):
    import wratio_ref
    X = list(frame(kind_of(m))[0])
    A, B = ([lit], X) if side == "a" else (X, [lit])
    if m == "wratio":
        return wratio_ref.Frames().columns(A, B)["wratio"]
    return models().sim(m, *RC.bcast(A, B))


@functools.lru_cache(maxsize=None)
def search_frames(name, v):
    """(queries, candidates) of a search, as the variant has them"""
    if name == "slow":
        Q, Cs = gen.batch_boundary_frame(11, "both")
    else:
        Q, Cs = F.token_search_frame() if name == "token" else F.search_frame()
    Q, Cs = list(Q), list(Cs)
    if v == "reversed":
        Q, Cs = Q[::-1], Cs[::-1]
    elif v == "empty_last":
        Q, Cs = Q + [""], Cs + [""]
    return tuple(Q), tuple(Cs)


@functools.lru_cache(maxsize=None)
def search_model(entry, m, name, v, cut):
    Q, Cs = search_frames(name, v)
    return getattr(models(), entry)(m, list(Q), list(Cs), K, cut)


@functools.lru_cache(maxsize=None)
def score_matrix(m, name, v):
    import cdist_ref
    Q, Cs = search_frames(name, v)
    return cdist_ref.score_matrix(m, Q, Cs)


@functools.lru_cache(maxsize=None)
def cluster_column(v):
    import cluster_frames
    X = list(cluster_frames.frame(41))
    return tuple(X[::-1] if v == "reversed" else X + [""] if v == "empty_last" else X)


@functools.lru_cache(maxsize=None)
def self_join_model(scorer, v, cut):
    import join_ref
    X = list(cluster_column(v))
    return join_ref.join(scorer, X, X, cut, True)


# ---- the buffer and the context ----

class Env:
    def __init__(self, S, torch, ctx, hb):
        self.S, self.torch, self.ctx, self.hb = S, torch, ctx, hb
        self.low = {}  # (what, variant) -> the counters of the call at base 0

    def columns(self, *placed):
        """(strings, placement) ... -> their device columns, all in the buffer at once"""
        self.hb.reset()
        out = ()
        for strings, name in placed:
            out += self.hb.place_named(list(strings), name)
        return out

    def out_column(self, rows, nbytes):
        """small output tensors of a transform: the wrappers' default is a multiple of values.numel(), the whole buffer here"""
        return (self.torch.empty(rows + 1, dtype=self.torch.int32, device="cuda:0"),
                self.torch.empty(max(nbytes, 1), dtype=self.torch.uint8, device="cuda:0"))

    def strings_of(self, off, val, rows):
        off = off.cpu().numpy().view(np.uint32)
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
        raw = val[:int(off[rows])].cpu().numpy().tobytes()
        return tuple(raw[int(off[i]):int(off[i + 1])].decode("utf-8") for i in range(rows))

    def plan(self, key, v, *placements):
        """The placements of a call to run: the one at base 0 first, where it has not been made yet -- it must equal the model like
        every other, and it files the counters the others are held to."""
        low = ("low",) * len(placements[0])
        return ([low] if (key, v) not in self.low else []) + [p for p in placements if tuple(p) != low] or [low]

    def counters_against_low(self, key, v, placements, counters=None, check=None):
        """The call at base 0 files its counters; every other placement must show the same (check: the bound of a classic call)."""
        counters = counters or {}
        if all(p == "low" for p in placements):
            self.low[(key, v)] = counters
            return
        low = self.low[(key, v)]
        if counters:
            print(key, v, placements, counters, "low:", low)
        if check is not None:
            check(counters, low)
        else:
            assert counters == low, (key, v, placements, counters, low)


@pytest.fixture(scope="module")
def env():
    import strsim_amd
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < H.MIN_FREE:
        pytest.skip("less than 8 GiB of device memory free")
    assert set(WEIGHTED) == set(strsim_amd.WEIGHTED_MEASURES)
    hb = H.HighBuffer(torch, "cuda:0")
    torch.cuda.synchronize()
    with strsim_amd.Context(0) as ctx:
        yield Env(strsim_amd, torch, ctx, hb)
    hb.close()


def same_bits(got, exp, what):
    got, exp = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, (what, "%d of %d differ" % (len(bad), got.size), [(tuple(i), float(got[tuple(i)]), float(exp[tuple(i)])) for i in bad[:6]])


def same_ints(got, exp, what):
    got, exp = np.asarray(got).astype(np.int64), np.asarray(exp).astype(np.int64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, "%d of %d differ" % (len(bad), got.size), [(tuple(i), int(got[tuple(i)]), int(exp[tuple(i)])) for i in bad[:6]])


def beyond_stage(A, B):
    """rows outside the lane class of the classic five, by construction"""
    A, B = RC.bcast(list(A), list(B))
    ok = lambda s: s.isascii() and len(s) <= LANE_STAGE_MAX_BYTES  # noqa: E731
    return sum(not (ok(a) and ok(b)) for a, b in zip(A, B))


def pair_counters(env, m):
    c = env.ctx
    if m in RC.CLASSIC or m == "all":
        return {"wave": c.last_wave_rows, "long": c.last_long_rows}
    if m in RC.NEWER:
        return {"wave": c.last_wave_rows}
    if m == "token_sort_ratio":
        return {"wave": c.last_wave_rows, "token_wave": c.last_token_wave_rows}
    if m == "token_set_ratio":
        return {"token_wave": c.last_token_wave_rows}
    return {"wratio": c.last_wratio_rows()} if m == "wratio" else {}


def classic_check(A, B, passes=1):
    """The classic counter may count rows whose 32-byte window crosses the column's end, which depends on the alignment: at most 64
    beyond the rows outside the lane class (the relation suite's bound); the rows beyond WAVE_CAP are what they are.  passes: the
    fused call adds up the counters of its five measures."""
    beyond = beyond_stage(A, B)

    def check(counters, low):
        assert counters["wave"] <= passes * (beyond + 64) and low["wave"] <= passes * (beyond + 64), (counters, low, beyond)
        assert counters["long"] == low["long"], (counters, low)
    return check


# ---- strsim_pairs_device ----

@pytest.mark.parametrize("pa,pb", H.PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("m", PAIR_MEASURES)
def test_pairs_device(env, m, pa, pb):
    fa, fb = frame(kind_of(m))
    for v in VARIANTS:
        A, B, exp = variant(fa, v), variant(fb, v), variant(sim_model(m), v)
        for qa, qb in env.plan(m, v, (pa, pb)):
            out = env.ctx.pairs_device(m, *env.columns((A, qa), (B, qb)))
            env.ctx.synchronize()
            same_bits(out.cpu().numpy(), exp, f"{m} {v} a at {qa}, b at {qb}")
            env.counters_against_low(m, v, (qa, qb), pair_counters(env, m), classic_check(A, B) if m in RC.CLASSIC else None)


@pytest.mark.parametrize("pa,pb", H.PAIRS, ids=PAIR_IDS)
def test_pairs_device_all(env, pa, pb):
    fa, fb = frame("pair")
    for v in VARIANTS:
        A, B = variant(fa, v), variant(fb, v)
        for qa, qb in env.plan("all", v, (pa, pb)):
            outs = env.ctx.pairs_device_all(*env.columns((A, qa), (B, qb)))
            env.ctx.synchronize()
            for m, out in zip(env.S.MEASURES, outs):
                same_bits(out.cpu().numpy(), variant(sim_model(m), v), f"{m} of the fused call, {v} a at {qa}, b at {qb}")
            env.counters_against_low("all", v, (qa, qb), pair_counters(env, "all"), classic_check(A, B, passes=5))


LITERALS = ("fadebc", "ab " * 30)  # lane class; beyond the lane tiers of the classic five and of OSA, thirty tokens


@pytest.mark.parametrize("side", ("a", "b"))
@pytest.mark.parametrize("lit", LITERALS, ids=("short", "long"))
@pytest.mark.parametrize("m", ("levenshtein", "jaro_winkler", "indel", "wratio"))
def test_pairs_device_literal_at_the_top(env, m, lit, side):
    """a one-row column that ends at 0xFFFFFFFF against the frame, which holds byte 2^31"""
    X = variant(frame(kind_of(m))[0], "forward")
    exp = variant(literal_model(m, lit, side), "forward")
    key = ("literal", m, lit, side)
    for px, pl in env.plan(key, "forward", ("sign_short", "top1")):
        x, l = (X, px), ([lit], pl)
        cols = env.columns(l, x) if side == "a" else env.columns(x, l)
        out = env.ctx.pairs_device(m, *cols)
        env.ctx.synchronize()
        same_bits(out.cpu().numpy(), exp, f"{m} literal {lit!r} as {side} at {pl}, the column at {px}")
        env.counters_against_low(key, "forward", (px, pl), pair_counters(env, m), classic_check(X, [lit]) if m in RC.CLASSIC else None)


# ---- strsim_distance_device, strsim_partial_alignment_device, strsim_qgram_device ----

@pytest.mark.parametrize("pa,pb", H.PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("bounded", (False, True), ids=("unbounded", "cutoff"))
@pytest.mark.parametrize("m", RC.DISTANCES)
def test_distance_device(env, m, bounded, pa, pb):
    k = RC.CUTOFFS[m][1] if bounded else None  # (the relation suite's batch cutoff)
    fa, fb = frame("pair")
    for v in VARIANTS:
        for qa, qb in env.plan(("distance", m, k), v, (pa, pb)):
            out = env.ctx.distance_device(m, *env.columns((variant(fa, v), qa), (variant(fb, v), qb)), k)
            env.ctx.synchronize()
            same_ints(out.cpu().numpy().view(np.uint32), variant(dist_model(m, k), v), f"{m} distance k={k} {v} a at {qa}, b at {qb}")
            env.counters_against_low(("distance", m, k), v, (qa, qb))


@pytest.mark.parametrize("pa,pb", H.PAIRS, ids=PAIR_IDS)
def test_partial_alignment_device(env, pa, pb):
    fa, fb = frame("pair/1")
    score, span = partial_model("pair/1")
    for v in VARIANTS:
        for qa, qb in env.plan("partial_alignment", v, (pa, pb)):
            s, p = env.ctx.partial_alignment_device(*env.columns((variant(fa, v), qa), (variant(fb, v), qb)))
            env.ctx.synchronize()
            same_bits(s.cpu().numpy(), variant(score, v), f"partial alignment score {v} a at {qa}, b at {qb}")
            same_ints(p.cpu().numpy().view(np.uint32), variant(span, v), f"partial alignment span {v} a at {qa}, b at {qb}")
            env.counters_against_low("partial_alignment", v, (qa, qb))


@pytest.mark.parametrize("pa,pb", H.PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("kind,q,multiset", QGRAMS)
def test_qgram_device(env, kind, q, multiset, pa, pb):
    fa, fb = frame("pair")
    key = ("qgram", kind, q, multiset)
    for v in VARIANTS:
        for qa, qb in env.plan(key, v, (pa, pb)):
            out = env.ctx.qgram_device(kind, *env.columns((variant(fa, v), qa), (variant(fb, v), qb)), q=q, multiset=multiset)
            env.ctx.synchronize()
            same_bits(out.cpu().numpy(), variant(qgram_model(kind, q, multiset), v), f"{kind} q={q} {v} a at {qa}, b at {qb}")
            env.counters_against_low(key, v, (qa, qb), {"wave": env.ctx.last_wave_rows})


# ---- the transforms and processed scoring ----

@pytest.mark.parametrize("place", H.PLACEMENTS)
@pytest.mark.parametrize("name", ("token_sort", "default_process"))
def test_transform_device(env, name, place):
    fx = frame("token")[0]
    for v in VARIANTS:
        X, exp = variant(fx, v), variant(transform_model(name), v)
        nbytes = int(H.byte_lengths(X).sum())
        for (p,) in env.plan(name, v, (place,)):
            off, val = env.columns((X, p))
            if name == "token_sort":
                o, w = env.ctx.token_sort_device(off, val, *env.out_column(len(X), nbytes))
            else:
                o, w = env.ctx.default_process_device(off, val, *env.out_column(len(X), nbytes + nbytes // 2))
            env.ctx.synchronize()
            assert env.strings_of(o, w, len(X)) == exp, f"{name} {v} at {p}"
            wave = env.ctx.last_token_wave_rows if name == "token_sort" else env.ctx.last_process_wave_rows
            env.counters_against_low(name, v, (p,), {"wave": wave})


@pytest.mark.parametrize("pa", H.PLACEMENTS)
@pytest.mark.parametrize("m", ("indel", "wratio"))
def test_pairs_processed_device(env, m, pa):
    fa, fb = frame("token/1" if m == "wratio" else "pair")
    for v in VARIANTS:
        for qa, qb in env.plan(("processed", m), v, (pa, PARTNER[pa])):
            out = env.ctx.pairs_processed_device(m, *env.columns((variant(fa, v), qa), (variant(fb, v), qb)))
            env.ctx.synchronize()
            same_bits(out.cpu().numpy(), variant(processed_model(m), v), f"processed {m} {v} a at {qa}, b at {qb}")
            counters = dict(pair_counters(env, m), process_wave=env.ctx.last_process_wave_rows)
            env.counters_against_low(("processed", m), v, (qa, qb), counters)


# ---- the searches ----

def search_device(env, entry, m, cols, nq, cut):
    from strsim_amd import _lib
    L, t = _lib.lib(), env.torch
    index = t.empty((nq, K), dtype=t.int32, device="cuda:0")
    if entry == "extract":
        index, value = env.ctx.extract(m, *cols, k=K, score_cutoff=cut)
    else:
        value = t.empty((nq, K), dtype=t.int32 if entry == "nearest" else t.float64, device="cuda:0")
        nc = cols[2].numel() - 1
        if entry == "nearest":
            bound = C.c_uint32(env.S.DISTANCE_UNBOUNDED if cut is None else cut)
        else:
            bound = C.c_double(-np.inf if cut is None else cut)
        _lib.check(getattr(L, "strsim_%s_device" % entry)(env.ctx._h, _lib.measure_id(m), cols[0].data_ptr(), cols[1].data_ptr(), nq, cols[2].data_ptr(),
                                                          cols[3].data_ptr(), nc, K, bound, index.data_ptr(), value.data_ptr()))
    env.ctx.synchronize()
    idx = index.cpu().numpy().view(np.uint32)
    val = value.cpu().numpy()
    val = val.view(np.uint32) if entry == "nearest" else val
    empty = idx == 0xFFFFFFFF
    assert np.array_equal(empty, np.isnan(val) if val.dtype == np.float64 else val == 0xFFFFFFFF)
    return np.where(empty, -1, idx.astype(np.int64)), (val if val.dtype == np.float64 else np.where(empty, -1, val.astype(np.int64)))


SEARCHES = [("best_match", "jaro_winkler"), ("best_match", "levenshtein"), ("nearest", "levenshtein"), ("nearest", "osa"),
            ("extract", "indel"), ("extract", "token_sort_ratio")]
SEARCH_CUT = {"best_match": F.BEST_MATCH_CUTOFF, "nearest": {"levenshtein": F.NEAREST_CUTOFF, "osa": F.NEAREST_CUTOFF}, "extract": F.EXTRACT_CUTOFF}


@pytest.mark.parametrize("pa,pb", H.PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", ("plain", "slow"))
@pytest.mark.parametrize("entry,m", SEARCHES)
def test_search_device(env, entry, m, name, pa, pb):
    """k = 3 with and without a cutoff; "slow": gen.batch_boundary_frame, whose fallback scores literals out of the placed columns"""
    if name == "plain" and m == "token_sort_ratio":
        name = "token"
    for v in VARIANTS:
        Q, Cs = search_frames(name, v)
        for cut in (SEARCH_CUT[entry][m], None):
            key = (entry, m, name, cut)
            for qa, qb in env.plan(key, v, (pa, pb)):
                got = search_device(env, entry, m, env.columns((Q, qa), (Cs, qb)), len(Q), cut)
                RC.same_lists(got, search_model(entry, m, name, v, cut), f"{entry} by {m} cutoff={cut} {name} {v} queries at {qa}, candidates at {qb}")
                env.counters_against_low(key, v, (qa, qb))


# ---- cdist, the joins, cluster ----

@pytest.mark.parametrize("pa", sorted(THREE))
@pytest.mark.parametrize("name", ("plain", "slow"))
@pytest.mark.parametrize("m", ("indel", "jaro"))
def test_cdist_device(env, m, name, pa):
    import cdist_ref
    for v in VARIANTS:
        Q, Cs = search_frames(name, v)
        for cut in (None, 0.6):
            key = ("cdist", m, name, cut)
            exp = cdist_ref.apply_cutoff(score_matrix("ratio" if m == "indel" else m, name, v), cut)
            for qa, qb in env.plan(key, v, (pa, THREE[pa])):
                out = env.ctx.cdist(m, *env.columns((Q, qa), (Cs, qb)), score_cutoff=cut)
                env.ctx.synchronize()
                same_bits(out.cpu().numpy(), exp, f"cdist by {m} cutoff={cut} {name} {v} queries at {qa}, candidates at {qb}")
                env.counters_against_low(key, v, (qa, qb))


def csr_of(got):
    indptr, index, score = got
    return indptr.cpu().numpy().view(np.uint64), index.cpu().numpy().view(np.uint32), score.cpu().numpy()


@pytest.mark.parametrize("pa", sorted(THREE))
@pytest.mark.parametrize("name", ("plain", "slow"))
def test_match_join_device(env, name, pa):
    import match_join_ref
    cut = F.BEST_MATCH_CUTOFF["jaro_winkler"]
    for v in VARIANTS:
        Q, Cs = search_frames(name, v)
        exp = match_join_ref.from_scores(score_matrix("jaro_winkler", name, v), cut, False)
        assert len(exp[1]) > 20
        for qa, qb in env.plan(("match_join", name), v, (pa, THREE[pa])):
            got = env.ctx.match_join("jaro_winkler", *env.columns((Q, qa), (Cs, qb)), min_score=cut)
            env.ctx.synchronize()
            assert match_join_ref.same(csr_of(got), exp), f"match_join {name} {v} queries at {qa}, candidates at {qb}"
            env.counters_against_low(("match_join", name), v, (qa, qb))


@pytest.mark.parametrize("place", sorted(THREE))
def test_self_join_and_cluster_device(env, place):
    """join by ratio with upper=True over ONE placed column, passed as both sides; cluster by ratio of the same column"""
    import cluster_frames
    import cluster_ref
    import join_ref
    cut = cluster_frames.MIN_SCORE["ratio"]
    for v in VARIANTS:
        X = cluster_column(v)
        exp = self_join_model("ratio", v, cut)
        model = cluster_ref.cluster("ratio", X, cut, exp)
        assert len(exp[1]) > 20 and 3 < model[2] < len(X) - 3
        for (p,) in env.plan("self_join", v, (place,)):
            off, val = env.columns((X, p))
            got = env.ctx.join("indel", off, val, off, val, score_cutoff=cut, upper=True)
            env.ctx.synchronize()
            assert join_ref.same(csr_of(got), exp), f"self-join {v} at {p}"
            root, cluster, count, nnz = env.ctx.cluster("indel", off, val, cut, with_nnz=True)
            env.ctx.synchronize()
            assert (root.cpu().tolist(), cluster.cpu().tolist(), count, nnz) == tuple(model), f"cluster {v} at {p}"
            env.counters_against_low("self_join", v, (p,))
