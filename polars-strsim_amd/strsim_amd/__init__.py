"""strsim_amd -- host side of the MI355X pairwise string-similarity path (above the C ABI).

`Context` wraps include/strsim_amd.h; the five functions below mirror the reference's operator surface
(polars_strsim/__init__.py:8-60: levenshtein / jaro / jaro_winkler / jaccard / sorensen_dice over two
string columns, either side may be a single literal) for plain Python / numpy inputs, so parity tests
read like the reference's own.  Nulls (None) propagate: null in -> null (NaN in the f64 array plus a
validity mask), as in README.md:69-70.
"""
import numpy as np

from ._lib import COMMON_KINDS, common_kind_id, EDIT_KINDS, edit_kind_id, PROCESSORS, QGRAM_KINDS, QGRAM_MAX_Q, qgram_args, DISTANCE_MEASURES, DISTANCE_UNBOUNDED, ENTRY_POINT_ID, EXTRA_MEASURES, INDEL_MEASURES, MEASURES, MEASURE_ID, PARTIAL_MEASURES, TOKEN_MEASURES, WEIGHTED_MEASURES, LIB_PATH, STATUS, ShapeMismatch, StrsimError, lib, processor_id
from .context import Codec, Context, device_count, pack_strings, split_offsets

_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def _as_column(x):
    """-> (list of str/bytes with None replaced by '', validity bool array or None)"""
    if isinstance(x, (str, bytes)) or x is None:
        x = [x]
    x = list(x)
    valid = np.array([v is not None for v in x], dtype=bool)
    vals = [v if v is not None else "" for v in x]
    return vals, (None if valid.all() else valid)


def similarity(measure, a, b, ctx=None, processor=None):
    """f64 numpy array (NaN where either input is null) for two columns / a column and a literal.  processor=None compares the
    strings as they are; "default_process" (PROCESSORS) first runs default_process() over both sides, on the GPU."""
    if processor is not None:
        processor_id(processor)
    ctx = ctx or default_context()
    A, va = _as_column(a)
    B, vb = _as_column(b)
    ao, av = pack_strings(A)
    bo, bv = pack_strings(B)
    out = ctx.pairs_host(measure, ao, av, bo, bv) if processor is None else ctx.pairs_processed_host(measure, ao, av, bo, bv, processor)
    out[_null_mask(out.size, va, vb)] = np.nan
    return out


def _null_mask(n, *validities):
    """Boolean array, True where a row of any input is null.  A validity of None has no nulls; one of a single row is a literal's."""
    mask = np.zeros(n, dtype=bool)
    for v in validities:
        if v is not None:
            mask |= ~(np.broadcast_to(v, (n,)) if v.size == 1 else v)
    return mask


def _pack_candidates(candidates):
    """The non-null candidates packed -> (offsets, values, pos: each packed candidate's position in `candidates`)."""
    cand = list(candidates)
    pos = np.flatnonzero(np.array([c is not None for c in cand], dtype=bool))
    return (*pack_strings([cand[j] for j in pos]), pos)


def _remap_candidates(idx, pos, query_valid):
    """Indices into the packed candidates -> int64 positions in the caller's list, -1 in empty slots and for null queries."""
    empty = idx == 0xFFFFFFFF
    out = np.full(idx.shape, -1, dtype=np.int64)
    out[~empty] = pos[idx[~empty].astype(np.int64)]
    if query_valid is not None:
        out[~query_valid] = -1
    return out


def levenshtein(a, b, ctx=None):
    return similarity("levenshtein", a, b, ctx)


def jaro(a, b, ctx=None):
    return similarity("jaro", a, b, ctx)


def jaro_winkler(a, b, ctx=None):
    return similarity("jaro_winkler", a, b, ctx)


def jaccard(a, b, ctx=None):
    return similarity("jaccard", a, b, ctx)


def sorensen_dice(a, b, ctx=None):
    return similarity("sorensen_dice", a, b, ctx)


def osa(a, b, ctx=None):
    """Optimal string alignment: the restricted Damerau-Levenshtein similarity.  Like levenshtein, with a swap of two adjacent
    characters counted as one edit; no substring is edited twice (("ca", "abc") is 3 edits, not the unrestricted variant's 2:
    damerau_levenshtein).  1.0 - d / max(len(a), len(b)) over characters, 1.0 when both are empty."""
    return similarity("osa", a, b, ctx)


def indel(a, b, ctx=None, processor=None):
    """Indel similarity: rapidfuzz's fuzz.ratio / 100 (Indel.normalized_similarity).  With l the length of the longest common
    subsequence, d = len(a) + len(b) - 2 l (insertions and deletions only: a substitution costs 2) and the score is
    1.0 - d / (len(a) + len(b)) over characters, 1.0 when both are empty."""
    return similarity("indel", a, b, ctx, processor)


def partial_ratio(a, b, ctx=None, processor=None):
    """Partial ratio: rapidfuzz's fuzz.partial_ratio / 100.  The best indel() score of the shorter string (the needle, m
    characters) against a window of the longer one: its proper prefixes of 1 .. m-1 characters, every substring of m characters,
    its proper suffixes (the needle slid over the longer string one step at a time, overhanging either end).  Equal lengths: the
    larger of the two directions.  1.0 when both are empty, 0.0 when exactly one is.  It can be LOWER than indel(a, b): when the
    lengths differ the whole longer string is not one of the windows.  It is the maximum at every needle length (rapidfuzz's
    heuristic for needles of more than 64 characters is not followed)."""
    return similarity("partial_ratio", a, b, ctx, processor)


def partial_ratio_alignment(a, b, ctx=None):
    """partial_ratio() with the window that won: (score f64 [N], span masked uint32 [N, 4]).  span = a_start, a_end, b_start,
    b_end, half open, in characters: the needle spans (0, its length), the other string's span is the winning window; among
    windows with the same score the one with the smallest end wins, then the smallest start.  For equal lengths a is the needle
    unless b as the needle scores strictly higher.  Both empty, or one empty: (0, 0, 0, 0).  Nulls: NaN and a masked row."""
    ctx = ctx or default_context()
    A, va = _as_column(a)
    B, vb = _as_column(b)
    ao, av = pack_strings(A)
    bo, bv = pack_strings(B)
    score, span = ctx.partial_alignment_host(ao, av, bo, bv)
    mask = _null_mask(score.size, va, vb)
    score[mask] = np.nan
    return score, np.ma.MaskedArray(span, mask=np.repeat(mask[:, None], 4, axis=1))


def token_sort_ratio(a, b, ctx=None, processor=None):
    """rapidfuzz's fuzz.token_sort_ratio / 100: indel() of the two strings with their tokens sorted, bit for bit.  Tokens are split
    at whitespace -- exactly Python's str.isspace set, 29 code points -- as str.split() does, sorted as Python sorts str (by code
    point, a proper prefix first) and joined with one space; duplicates are kept.  Two strings without tokens give 1.0, exactly
    one gives 0.0.  No lower-casing and no other pre-processing."""
    return similarity("token_sort_ratio", a, b, ctx, processor)


def token_set_ratio(a, b, ctx=None, processor=None):
    """rapidfuzz's fuzz.token_set_ratio / 100 over the SETS of tokens (split as for token_sort_ratio): 0.0 when either string has
    no token, 1.0 when the sets share a token and one contains the other, else the best indel() among the pairs of
    sect, sect + " " + ab and sect + " " + ba -- the joined sorted intersection and the two differences."""
    return similarity("token_set_ratio", a, b, ctx, processor)


def token_ratio(a, b, ctx=None, processor=None):
    """rapidfuzz's fuzz.token_ratio / 100: max(token_sort_ratio(a, b), token_set_ratio(a, b))."""
    return similarity("token_ratio", a, b, ctx, processor)


def partial_token_sort_ratio(a, b, ctx=None, processor=None):
    """rapidfuzz's fuzz.partial_token_sort_ratio / 100: partial_ratio() of the two strings with their tokens sorted (split, sorted
    and joined as for token_sort_ratio)."""
    return similarity("partial_token_sort_ratio", a, b, ctx, processor)


def partial_token_set_ratio(a, b, ctx=None, processor=None):
    """rapidfuzz's fuzz.partial_token_set_ratio / 100 over the SETS of tokens: 0.0 when either string has no token, 1.0 when the
    sets share a token, else partial_ratio() of the joined sorted differences."""
    return similarity("partial_token_set_ratio", a, b, ctx, processor)


def partial_token_ratio(a, b, ctx=None, processor=None):
    """rapidfuzz's fuzz.partial_token_ratio / 100: max(partial_token_sort_ratio(a, b), partial_token_set_ratio(a, b))."""
    return similarity("partial_token_ratio", a, b, ctx, processor)


def wratio(a, b, ctx=None, processor=None):
    """rapidfuzz's fuzz.WRatio / 100 (the default scorer of process.extract), without a processor.  With lo, hi the shorter and
    the longer length in characters and r = indel(a, b): 0.0 when lo == 0; when 2 hi < 3 lo: max(r, token_ratio * 0.95);
    otherwise, with ps = 0.9 when hi <= 8 lo and 0.6 beyond: max(r, partial_ratio * ps, (partial_token_ratio * 0.95) * ps).
    The rows are classified on the GPU and each family runs over its own rows only (Context.last_wratio_rows())."""
    return similarity("wratio", a, b, ctx, processor)


def token_sort(col, ctx=None):
    """The normalisation of token_sort_ratio on its own: a list of str or None -> a list of str or None, each string
    " ".join(sorted(s.split())) computed on the GPU.  indel(token_sort(a), token_sort(b)) is token_sort_ratio(a, b); best_match
    and nearest over normalised columns search without regard to token order."""
    ctx = ctx or default_context()
    X, valid = _as_column(col)
    off, val = ctx.token_sort_host(*pack_strings(X))
    raw = val.tobytes()
    out = [raw[int(off[i]):int(off[i + 1])].decode("utf-8") for i in range(len(X))]
    if valid is not None:
        out = [s if ok else None for s, ok in zip(out, valid)]
    return out


def default_process(col, ctx=None):
    """rapidfuzz's utils.default_process on the GPU: a list of str or None -> a list of str or None.  Every character that is
    neither alphanumeric nor "_" becomes a space, the others are lower-cased, and spaces are removed from both ends; inner runs of
    spaces stay ("Apple, Inc." -> "apple  inc").  Character by character: U+03A3 is U+03C3 in every position and U+0130 is "i".
    indel(default_process(a), default_process(b)) is indel(a, b, processor="default_process")."""
    ctx = ctx or default_context()
    X, valid = _as_column(col)
    off, val = ctx.default_process_host(*pack_strings(X))
    raw = val.tobytes()
    out = [raw[int(off[i]):int(off[i + 1])].decode("utf-8") for i in range(len(X))]
    if valid is not None:
        out = [s if ok else None for s, ok in zip(out, valid)]
    return out


def measure_supported(measure, entry_point="pairwise"):
    """True if the library's `entry_point` ("pairwise", "best_match" or "codec") accepts `measure`; needs no device."""
    from ._lib import measure_id
    return bool(lib().strsim_measure_supported(measure_id(measure), ENTRY_POINT_ID[entry_point]))


def distance(measure, a, b, max_distance=None, ctx=None):
    """Integer edit distance ("levenshtein" or "osa", DISTANCE_MEASURES, or "indel", INDEL_MEASURES: insertions and deletions
    only, len(a) + len(b) - 2 LCS) over characters, for two columns / a column and a
    literal -> numpy.ma.MaskedArray of uint32, masked where either input is null.  With max_distance=k a row is d when d <= k and
    k + 1 otherwise (rapidfuzz's score_cutoff convention); None is no cutoff."""
    if measure not in DISTANCE_MEASURES + INDEL_MEASURES:
        raise ValueError(f"no distance for measure {measure!r} (one of {DISTANCE_MEASURES + INDEL_MEASURES})")
    ctx = ctx or default_context()
    A, va = _as_column(a)
    B, vb = _as_column(b)
    ao, av = pack_strings(A)
    bo, bv = pack_strings(B)
    out = ctx.distance_host(measure, ao, av, bo, bv, max_distance)
    return np.ma.MaskedArray(out, mask=_null_mask(out.size, va, vb))


def qgram(kind, a, b, q=2, multiset=True, ctx=None):
    """q-gram similarity of two columns / a column and a literal -> f64 numpy array, NaN where either input is null.  kind is one
    of QGRAM_KINDS, over the grams (q consecutive characters, q = 1, 2 or 3) of the two strings: with I the grams in common and
    na, nb the grams of each, "jaccard" is I / (na + nb - I), "sorensen_dice" 2 I / (na + nb), "overlap" I / min(na, nb) and
    "cosine" I / sqrt(na nb).  multiset=True counts a repeated gram as often as it occurs (I = sum of min(count_a, count_b)),
    False compares the sets of distinct grams.  Equal strings score 1.0, also when they are shorter than q; otherwise a string
    without a gram scores 0.0.  At q = 1 the first two are jaccard() and sorensen_dice()."""
    qgram_args(kind, q, multiset)
    ctx = ctx or default_context()
    A, va = _as_column(a)
    B, vb = _as_column(b)
    ao, av = pack_strings(A)
    bo, bv = pack_strings(B)
    out = ctx.qgram_host(kind, ao, av, bo, bv, q, multiset)
    out[_null_mask(out.size, va, vb)] = np.nan
    return out


def levenshtein_distance(a, b, max_distance=None, ctx=None):
    """Levenshtein distance (insert, delete, substitute) over characters; see distance()."""
    return distance("levenshtein", a, b, max_distance, ctx)


def osa_distance(a, b, max_distance=None, ctx=None):
    """Optimal string alignment distance (Levenshtein plus the restricted swap of two adjacent characters); see distance()."""
    return distance("osa", a, b, max_distance, ctx)


def indel_distance(a, b, max_distance=None, ctx=None):
    """Indel distance: len(a) + len(b) - 2 LCS(a, b) over characters (insert and delete, a substitution costs 2); see distance()."""
    return distance("indel", a, b, max_distance, ctx)


def _damerau_columns(a, b, max_distance=None):
    """The packed columns and validities of a damerau call; every ValueError of its arguments, before a context is touched."""
    from .context import _max_distance
    _max_distance(max_distance)
    A, va = _as_column(a)
    B, vb = _as_column(b)
    if len(A) != len(B) and len(A) != 1 and len(B) != 1:
        raise ShapeMismatch(1, f"Inputs must have the same length or one of them must be a literal (got {len(A)} and {len(B)} rows)")
    return pack_strings(A), pack_strings(B), va, vb


def damerau_levenshtein(a, b, ctx=None):
    """Unrestricted Damerau-Levenshtein similarity (strsim's normalized_damerau_levenshtein, rapidfuzz's
    DamerauLevenshtein.normalized_similarity) of two columns / a column and a literal -> f64 numpy array, NaN where either input
    is null.  d is the smallest number of insertions, deletions, substitutions and swaps of two adjacent characters, where a
    substring may be edited again after a swap: ("ca", "abc") is 2, where osa() counts 3.  Unlike osa's, this distance is a metric.
    1.0 - d / max(len(a), len(b)) over characters, 1.0 when both are empty."""
    (ao, av), (bo, bv), va, vb = _damerau_columns(a, b)
    ctx = ctx or default_context()
    out = ctx.damerau_host(ao, av, bo, bv)
    out[_null_mask(out.size, va, vb)] = np.nan
    return out


def damerau_levenshtein_distance(a, b, max_distance=None, ctx=None):
    """Unrestricted Damerau-Levenshtein distance over characters (see damerau_levenshtein) -> numpy.ma.MaskedArray of uint32,
    masked where either input is null.  max_distance as for distance().  levenshtein_distance >= osa_distance >= this >= the
    difference of the lengths, row by row."""
    (ao, av), (bo, bv), va, vb = _damerau_columns(a, b, max_distance)
    ctx = ctx or default_context()
    out = ctx.damerau_distance_host(ao, av, bo, bv, max_distance)
    return np.ma.MaskedArray(out, mask=_null_mask(out.size, va, vb))


def _char_lengths(offsets, values):
    """Unicode scalar values of every row of a packed column: the bytes that are not continuation bytes."""
    starts = np.concatenate(([0], np.cumsum((values & 0xC0) != 0x80, dtype=np.int64)))
    return starts[offsets[1:].astype(np.int64)] - starts[offsets[:-1].astype(np.int64)]


def _common(kind, out, a, b, max_distance=None, pad=True, ctx=None):
    """One of the twelve functions below: out is "similarity" (f64, NaN under nulls), "distance" or "count" (masked uint32).
    pad=False (Hamming): rows whose character counts differ are nulls too, decided here from the inputs."""
    common_kind_id(kind)
    (ao, av), (bo, bv), va, vb = _damerau_columns(a, b, max_distance)
    ctx = ctx or default_context()
    if out == "similarity":
        res = ctx.common_host(kind, ao, av, bo, bv)
    elif out == "distance":
        res = ctx.common_distance_host(kind, ao, av, bo, bv, max_distance)
    else:
        res = ctx.common_count_host(kind, ao, av, bo, bv)
    mask = _null_mask(res.size, va, vb)
    if not pad:
        mask = mask | np.broadcast_to(_char_lengths(ao, av) != _char_lengths(bo, bv), mask.shape)
    if out == "similarity":
        res[mask] = np.nan
        return res
    return np.ma.MaskedArray(res, mask=mask)


def hamming(a, b, pad=True, ctx=None):
    """Normalised Hamming similarity (rapidfuzz's Hamming.normalized_similarity) of two columns / a column and a literal -> f64
    numpy array, NaN where either input is null: 1 - hamming_distance / max(len(a), len(b)) over characters, 1.0 when both are
    empty.  pad=True (rapidfuzz's default) counts the difference of the lengths as mismatches; with pad=False a row whose strings
    differ in length is NaN (rapidfuzz raises there, which a column call cannot do per row)."""
    return _common("hamming", "similarity", a, b, None, pad, ctx)


def hamming_distance(a, b, max_distance=None, pad=True, ctx=None):
    """Hamming distance (strsim's hamming, rapidfuzz's Hamming.distance): the positions at which the two strings differ, over
    characters, plus the difference of their lengths -> numpy.ma.MaskedArray of uint32, masked where either input is null and,
    with pad=False, where the lengths differ.  max_distance as for distance()."""
    return _common("hamming", "distance", a, b, max_distance, pad, ctx)


def hamming_similarity(a, b, pad=True, ctx=None):
    """The positions at which the two strings agree (rapidfuzz's Hamming.similarity) -> masked uint32, as hamming_distance."""
    return _common("hamming", "count", a, b, None, pad, ctx)


def lcs_seq(a, b, ctx=None):
    """Normalised LCSseq similarity (rapidfuzz's LCSseq.normalized_similarity): l / max(len(a), len(b)) written as
    1 - (max(len) - l) / max(len), with l the length of the longest common subsequence over characters; 1.0 when both are empty.
    Not indel(), which is 2 l / (len(a) + len(b)).  f64, NaN where either input is null."""
    return _common("lcs_seq", "similarity", a, b, ctx=ctx)


def lcs_seq_distance(a, b, max_distance=None, ctx=None):
    """max(len(a), len(b)) minus the length of the longest common subsequence (rapidfuzz's LCSseq.distance) -> masked uint32.
    max_distance as for distance().  hamming_distance >= levenshtein_distance >= this, row by row."""
    return _common("lcs_seq", "distance", a, b, max_distance, ctx=ctx)


def lcs_seq_similarity(a, b, ctx=None):
    """The length of the longest common subsequence over characters (rapidfuzz's LCSseq.similarity) -> masked uint32."""
    return _common("lcs_seq", "count", a, b, ctx=ctx)


def prefix(a, b, ctx=None):
    """Normalised common-prefix similarity (rapidfuzz's Prefix.normalized_similarity): the length of the longest common prefix
    over characters, divided by max(len(a), len(b)); 1.0 when both are empty.  f64, NaN where either input is null."""
    return _common("prefix", "similarity", a, b, ctx=ctx)


def prefix_distance(a, b, max_distance=None, ctx=None):
    """max(len(a), len(b)) minus the length of the longest common prefix (rapidfuzz's Prefix.distance) -> masked uint32.
    max_distance as for distance()."""
    return _common("prefix", "distance", a, b, max_distance, ctx=ctx)


def prefix_similarity(a, b, ctx=None):
    """The length of the longest common prefix over characters (rapidfuzz's Prefix.similarity) -> masked uint32."""
    return _common("prefix", "count", a, b, ctx=ctx)


def postfix(a, b, ctx=None):
    """Normalised common-suffix similarity (rapidfuzz's Postfix.normalized_similarity): the length of the longest common suffix
    over characters, divided by max(len(a), len(b)); 1.0 when both are empty.  f64, NaN where either input is null."""
    return _common("postfix", "similarity", a, b, ctx=ctx)


def postfix_distance(a, b, max_distance=None, ctx=None):
    """max(len(a), len(b)) minus the length of the longest common suffix (rapidfuzz's Postfix.distance) -> masked uint32.
    max_distance as for distance()."""
    return _common("postfix", "distance", a, b, max_distance, ctx=ctx)


def postfix_similarity(a, b, ctx=None):
    """The length of the longest common suffix over characters (rapidfuzz's Postfix.similarity) -> masked uint32."""
    return _common("postfix", "count", a, b, ctx=ctx)


def best_match(measure, queries, candidates, k=1, min_score=None, ctx=None):
    """For every query, its k best candidates by `measure`: (index int64 [N, k], score f64 [N, k]).  Slots in descending order
    of the score, ties to the lower candidate index; a candidate below min_score is not reported.  Empty slots -- and every slot
    of a null query -- are (-1, NaN).  Null candidates are never matched; indices refer to the caller's candidate positions."""
    if measure in INDEL_MEASURES + PARTIAL_MEASURES + TOKEN_MEASURES + WEIGHTED_MEASURES:
        raise ValueError(f"no best match by measure {measure!r} (one of {MEASURES})")
    ctx = ctx or default_context()
    Q, vq = _as_column(queries)
    qo, qv = pack_strings(Q)
    co, cv, pos = _pack_candidates(candidates)
    idx, score = ctx.best_match(measure, qo, qv, co, cv, k, min_score)
    out = _remap_candidates(idx, pos, vq)
    if vq is not None:
        score[~vq] = np.nan
    return out, score


def nearest(measure, queries, candidates, k=1, max_distance=None, ctx=None):
    """For every query, its k nearest candidates by edit distance ("levenshtein" or "osa", DISTANCE_MEASURES):
    (index int64 [N, k], distance int64 [N, k]).  Slots in ascending order of the distance, ties to the lower candidate index;
    only candidates within max_distance are reported (None: no cutoff, 0: exact matches).  Empty slots -- and every slot of a
    null query -- are (-1, -1).  Null candidates are never matched; indices refer to the caller's candidate positions.
    rapidfuzz: process.extract(q, candidates, scorer=Levenshtein.distance, score_cutoff=max_distance, limit=k)."""
    if measure not in DISTANCE_MEASURES:
        raise ValueError(f"no distance for measure {measure!r} (one of {DISTANCE_MEASURES})")
    ctx = ctx or default_context()
    Q, vq = _as_column(queries)
    qo, qv = pack_strings(Q)
    co, cv, pos = _pack_candidates(candidates)
    idx, dist = ctx.nearest(measure, qo, qv, co, cv, k, max_distance)
    out = _remap_candidates(idx, pos, vq)
    return out, np.where(out < 0, -1, dist.astype(np.int64))


EXTRACT_SCORERS = ("ratio", "token_sort_ratio")
_EXTRACT_SCORER_MEASURE = {"ratio": "indel", "indel": "indel", "token_sort_ratio": "token_sort_ratio"}


def extract(scorer, queries, candidates, k=1, score_cutoff=None, ctx=None, processor=None):
    """For every query, its k best candidates by `scorer` ("ratio" -- "indel" is an alias -- or "token_sort_ratio",
    EXTRACT_SCORERS): (index int64 [N, k], score f64 [N, k]).  The score is indel(q, c) or token_sort_ratio(q, c), in [0, 1], bit
    for bit the pairwise call's.  Slots in descending order of the score, ties to the lower candidate index; a candidate below
    score_cutoff is not reported (None: no cutoff).  Empty slots -- and every slot of a null query -- are (-1, NaN).  Null
    candidates are never matched; indices refer to the caller's candidate positions.
    rapidfuzz: process.extract(q, candidates, scorer=fuzz.ratio, score_cutoff=100 * score_cutoff, limit=k), scores / 100.
    processor="default_process" runs default_process() over the queries and the candidates on the GPU and searches those
    (rapidfuzz's processor=utils.default_process)."""
    if scorer not in _EXTRACT_SCORER_MEASURE:
        raise ValueError(f"no extract by scorer {scorer!r} (one of {EXTRACT_SCORERS})")
    if processor is not None:
        processor_id(processor)
    ctx = ctx or default_context()
    Q, vq = _as_column(queries)
    qo, qv = pack_strings(Q)
    co, cv, pos = _pack_candidates(candidates)
    if processor is not None:
        qo, qv = ctx.default_process_host(qo, qv)
        co, cv = ctx.default_process_host(co, cv)
    idx, score = ctx.extract(_EXTRACT_SCORER_MEASURE[scorer], qo, qv, co, cv, k, score_cutoff)
    out = _remap_candidates(idx, pos, vq)
    if vq is not None:
        score[~vq] = np.nan
    return out, score


CDIST_MEASURES = MEASURES + ("ratio", "token_sort_ratio")
_CDIST_MEASURE = {**{m: m for m in MEASURES}, "ratio": "indel", "indel": "indel", "token_sort_ratio": "token_sort_ratio"}


def cdist(measure, queries, candidates, score_cutoff=None, ctx=None, processor=None):
    """The full score matrix of queries x candidates by `measure` (one of the reference measures, "ratio" -- "indel" is an alias
    -- or "token_sort_ratio", CDIST_MEASURES): f64 [N, M], element (i, j) the score of (queries[i], candidates[j]) in [0, 1], bit
    for bit the pairwise call's, in the caller's candidate positions.  A score below score_cutoff is 0.0 (None: no cutoff).  The
    row of a null query is NaN and the column of a null candidate is NaN.
    rapidfuzz: process.cdist(queries, candidates, scorer=fuzz.ratio, score_cutoff=100 * score_cutoff) / 100.
    processor="default_process" runs default_process() over the queries and the candidates on the GPU first (rapidfuzz's
    processor=utils.default_process)."""
    if not isinstance(measure, str) or measure not in _CDIST_MEASURE:
        raise ValueError(f"no cdist by measure {measure!r} (one of {CDIST_MEASURES})")
    if processor is not None:
        processor_id(processor)
    ctx = ctx or default_context()
    Q, vq = _as_column(queries)
    qo, qv = pack_strings(Q)
    cand = list(candidates)
    co, cv, pos = _pack_candidates(cand)
    if processor is not None:
        qo, qv = ctx.default_process_host(qo, qv)
        co, cv = ctx.default_process_host(co, cv)
    out = np.full((len(Q), len(cand)), np.nan, dtype=np.float64)
    if len(Q) and len(pos):
        out[:, pos] = ctx.cdist(_CDIST_MEASURE[measure], qo, qv, co, cv, score_cutoff)
    if vq is not None:
        out[~vq] = np.nan
    return out


JOIN_SCORERS = ("ratio", "token_sort_ratio")
_JOIN_SCORER_MEASURE = _EXTRACT_SCORER_MEASURE


def join(scorer, queries, candidates, score_cutoff, upper=False, ctx=None, processor=None):
    """Threshold join: every pair (query i, candidate j) whose score by `scorer` ("ratio" -- "indel" is an alias -- or
    "token_sort_ratio", JOIN_SCORERS) is >= score_cutoff, as CSR: (indptr int64 [N + 1], index int64 [nnz], score f64 [nnz]).  The
    hits of query i are index / score[indptr[i]:indptr[i + 1]], in ascending candidate position; the score is in [0, 1], bit for bit
    the pairwise call's.  Nothing is truncated: a query with 40 duplicates has 40 hits.  score_cutoff=None reports every pair.
    upper=True reports only j > i: with the same list on both sides that is each unordered pair once, never a row with itself
    (dedupe_pairs).  A null query has an empty row and null candidates are never matched; indices refer to the caller's candidate
    positions.  processor="default_process" runs default_process() over both sides on the GPU first.
    rapidfuzz: the pairs process.cdist(queries, candidates, scorer=fuzz.ratio, score_cutoff=100 * score_cutoff) leaves non-zero."""
    if not isinstance(scorer, str) or scorer not in _JOIN_SCORER_MEASURE:
        raise ValueError(f"no join by scorer {scorer!r} (one of {JOIN_SCORERS})")
    return _join_lists(lambda c: c.join, _JOIN_SCORER_MEASURE[scorer], queries, candidates, score_cutoff, upper, ctx, processor)


def _join_lists(call, measure, queries, candidates, cutoff, upper, ctx, processor, value_dtype=np.float64):
    """join(), match_join(), qgram_join() and distance_join() over Python lists: call(ctx) is the context's method; nulls, `upper`
    and the processor alike.  value_dtype: of the value a hit carries (the f64 score, or the uint32 distance)"""
    if processor is not None:
        processor_id(processor)
    ctx = ctx or default_context()
    Q, vq = _as_column(queries)
    qo, qv = pack_strings(Q)
    cand = list(candidates)
    if upper:
        # j > i compares positions: the null candidates keep theirs (as empty strings) and their hits are dropped below
        vc = np.array([c is not None for c in cand], dtype=bool)
        co, cv = pack_strings([c if c is not None else "" for c in cand])
        pos = np.arange(len(cand), dtype=np.int64)
    else:
        vc = None
        co, cv, pos = _pack_candidates(cand)
    if processor is not None:
        qo, qv = ctx.default_process_host(qo, qv)
        co, cv = ctx.default_process_host(co, cv)
    indptr, idx, score = call(ctx)(measure, qo, qv, co, cv, cutoff, upper)
    indptr = np.asarray(indptr).astype(np.int64)
    index = pos[np.asarray(idx).astype(np.int64)] if len(idx) else np.zeros(0, dtype=np.int64)
    score = np.asarray(score, dtype=value_dtype)
    keep = np.ones(index.size, dtype=bool)
    rows = np.repeat(np.arange(len(Q), dtype=np.int64), np.diff(indptr))
    if vq is not None:
        keep &= vq[rows]
    if vc is not None and not vc.all():
        keep &= vc[index]
    if not keep.all():
        index, score = index[keep], score[keep]
        indptr = np.concatenate(([0], np.cumsum(np.bincount(rows[keep], minlength=len(Q))))).astype(np.int64)
    return indptr, index, score


def dedupe_pairs(scorer, column, score_cutoff, ctx=None, processor=None):
    """The near-duplicates of one column: the self-join join(scorer, column, column, score_cutoff, upper=True) as COO -- (i int64
    [nnz], j int64 [nnz], score f64 [nnz]) with i < j, every unordered pair at or above score_cutoff once, ordered by i, then j."""
    column = list(column)
    indptr, index, score = join(scorer, column, column, score_cutoff, upper=True, ctx=ctx, processor=processor)
    return np.repeat(np.arange(len(column), dtype=np.int64), np.diff(indptr)), index, score


MATCH_JOIN_MEASURES = MEASURES


def match_join(measure, queries, candidates, min_score, upper=False, ctx=None, processor=None):
    """Threshold join by one of the five reference measures (MATCH_JOIN_MEASURES): every pair (query i, candidate j) whose score
    by `measure` is >= min_score, as CSR: (indptr int64 [N + 1], index int64 [nnz], score f64 [nnz]) -- "every pair of names with
    Jaro-Winkler >= 0.9" without cdist's N x M matrix and without best_match's limit on k.  The hits of query i are index /
    score[indptr[i]:indptr[i + 1]], in ascending candidate position; the score is bit for bit the pairwise call's.  min_score=None
    reports every pair.  upper, the nulls and processor="default_process" are join()'s."""
    if not isinstance(measure, str) or measure not in MATCH_JOIN_MEASURES:
        raise ValueError(f"no match_join by measure {measure!r} (one of {MATCH_JOIN_MEASURES})")
    return _join_lists(lambda c: c.match_join, measure, queries, candidates, min_score, upper, ctx, processor)


def match_dedupe_pairs(measure, column, min_score, ctx=None, processor=None):
    """The near-duplicates of one column by a reference measure: the self-join match_join(measure, column, column, min_score,
    upper=True) as COO -- (i int64 [nnz], j int64 [nnz], score f64 [nnz]) with i < j, ordered by i, then j."""
    column = list(column)
    indptr, index, score = match_join(measure, column, column, min_score, upper=True, ctx=ctx, processor=processor)
    return np.repeat(np.arange(len(column), dtype=np.int64), np.diff(indptr)), index, score


def qgram_join(kind, queries, candidates, min_score, q=2, multiset=True, upper=False, ctx=None, processor=None):
    """Threshold join by q-gram similarity: every pair (query i, candidate j) whose qgram(kind, q, multiset) score is >= min_score,
    as CSR: (indptr int64 [N + 1], index int64 [nnz], score f64 [nnz]) -- "which rows look like which, at bigram Dice 0.8 or
    better" (pg_trgm's similarity join, strsim's sorensen_dice over a whole column).  kind is one of QGRAM_KINDS, q is 1, 2 or 3,
    multiset=False compares the sets of grams.  The hits of query i are index / score[indptr[i]:indptr[i + 1]], in ascending
    candidate position; the score is bit for bit qgram()'s.  min_score=None reports every pair.  upper, the nulls and
    processor="default_process" are join()'s."""
    qgram_args(kind, q, multiset)
    call = lambda c: lambda _, qo, qv, co, cv, cut, up: c.qgram_join(kind, qo, qv, co, cv, cut, up, q=q, multiset=multiset)
    return _join_lists(call, kind, queries, candidates, min_score, upper, ctx, processor)


def qgram_dedupe_pairs(kind, column, min_score, q=2, multiset=True, ctx=None, processor=None):
    """The near-duplicates of one column by q-gram similarity: the self-join qgram_join(kind, column, column, min_score, q,
    multiset, upper=True) as COO -- (i int64 [nnz], j int64 [nnz], score f64 [nnz]) with i < j, ordered by i, then j."""
    column = list(column)
    indptr, index, score = qgram_join(kind, column, column, min_score, q, multiset, upper=True, ctx=ctx, processor=processor)
    return np.repeat(np.arange(len(column), dtype=np.int64), np.diff(indptr)), index, score


CLUSTER_MEASURES = MEASURES + ("ratio", "token_sort_ratio")
_CLUSTER_MEASURE = {**{m: m for m in MEASURES}, "ratio": "indel", "indel": "indel", "token_sort_ratio": "token_sort_ratio"}


def components(indptr, index, rows=None, ctx=None):
    """Connected components of a CSR graph, its edges read as undirected (the CSR of join(..., upper=True) as it is): (root int64
    [rows], cluster int64 [rows], count).  root[v] is the smallest row of v's component, cluster[v] the number of roots below it --
    the clusters are numbered 0 .. count - 1 in order of their first member -- and a row without an edge is a cluster of one."""
    ctx = ctx or default_context()
    root, cluster, count = ctx.components(np.asarray(indptr), np.asarray(index), rows)
    return root.astype(np.int64), cluster.astype(np.int64), count


def cluster(measure, column, min_score, ctx=None, processor=None):
    """The duplicate groups of one column: the rows that score >= min_score by `measure` (CLUSTER_MEASURES; "indel" is an alias of
    "ratio") are linked and the connected components of the links are the clusters -> (root int64 [n], cluster int64 [n], count).
    root[r] is the position of the first member of r's cluster, cluster[r] numbers the clusters 0 .. count - 1 in order of their
    first member.  Components chain: a ~ b and b ~ c put a and c together even where a and c do not match each other.  The pairs of
    the self-join stay on the GPU.  A null row never joins anything: its root and cluster are -1 and it is not counted.
    min_score=None is refused (it would put every row in one cluster).  processor="default_process" as in join()."""
    if not isinstance(measure, str) or measure not in _CLUSTER_MEASURE:
        raise ValueError(f"no cluster by measure {measure!r} (one of {CLUSTER_MEASURES})")
    return _cluster_column(lambda c, o, v: c.cluster(_CLUSTER_MEASURE[measure], o, v, min_score), column, min_score, ctx, processor)


def _cluster_column(call, column, min_score, ctx, processor, cutoff="min_score", advice="a score in [0, 1]"):
    """cluster(), qgram_cluster() and distance_cluster() over a Python list: call(ctx, offsets, values) is the context's method with
    its measure bound; min_score is only looked at for None (cutoff: its name in the refusal, advice: what to pass instead)"""
    if min_score is None:
        raise ValueError(f"cluster: {cutoff}=None would put every row in one cluster; pass {advice}")
    if processor is not None:
        processor_id(processor)
    ctx = ctx or default_context()
    column = list(column)
    pos = np.flatnonzero(np.array([c is not None for c in column], dtype=bool))  # the nulls are dropped, never kept as ""
    root = np.full(len(column), -1, dtype=np.int64)
    label = np.full(len(column), -1, dtype=np.int64)
    if not len(pos):
        return root, label, 0
    o, v = pack_strings([column[j] for j in pos])
    if processor is not None:
        o, v = ctx.default_process_host(o, v)
    r, c, count = call(ctx, o, v)
    root[pos] = pos[np.asarray(r).astype(np.int64)]
    label[pos] = np.asarray(c).astype(np.int64)
    return root, label, count


def qgram_cluster(kind, column, min_score, q=2, multiset=True, ctx=None, processor=None):
    """The duplicate groups of one column by q-gram similarity: cluster() with the rows linked that score >= min_score by
    qgram(kind, q, multiset) -> (root int64 [n], cluster int64 [n], count).  Components chain, a null row is -1 and not counted,
    min_score=None is refused, processor="default_process" as in join()."""
    qgram_args(kind, q, multiset)
    return _cluster_column(lambda c, o, v: c.qgram_cluster(kind, o, v, min_score, q=q, multiset=multiset), column, min_score, ctx, processor)


DISTANCE_JOIN_MEASURES = EDIT_KINDS


def distance_join(measure, queries, candidates, max_distance, upper=False, ctx=None, processor=None):
    """Join by integer edit distance: every pair (query i, candidate j) within max_distance edits by `measure` ("levenshtein",
    "osa" or "damerau_levenshtein": DISTANCE_JOIN_MEASURES), as CSR: (indptr int64 [N + 1], index int64 [nnz], distance uint32
    [nnz]) -- "which rows are within 2 edits of which".  The hits of query i are index / distance[indptr[i]:indptr[i + 1]], in
    ascending candidate position; the distance is exactly levenshtein_distance() / osa_distance() /
    damerau_levenshtein_distance() of the pair.  max_distance=0 is the exact-duplicate join, None reports every pair.  upper, the
    nulls and processor="default_process" are join()'s."""
    edit_kind_id(measure)
    call = lambda c: lambda kind, qo, qv, co, cv, k, up: c.distance_join(kind, qo, qv, co, cv, k, up)
    return _join_lists(call, measure, queries, candidates, max_distance, upper, ctx, processor, value_dtype=np.uint32)


def distance_dedupe_pairs(measure, column, max_distance, ctx=None, processor=None):
    """The near-duplicates of one column by edit distance: the self-join distance_join(measure, column, column, max_distance,
    upper=True) as COO -- (i int64 [nnz], j int64 [nnz], distance uint32 [nnz]) with i < j, ordered by i, then j."""
    column = list(column)
    indptr, index, dist = distance_join(measure, column, column, max_distance, upper=True, ctx=ctx, processor=processor)
    return np.repeat(np.arange(len(column), dtype=np.int64), np.diff(indptr)), index, dist


def distance_cluster(measure, column, max_distance, ctx=None, processor=None):
    """The duplicate groups of one column by edit distance: cluster() with the rows linked that are within max_distance edits by
    `measure` (DISTANCE_JOIN_MEASURES) -> (root int64 [n], cluster int64 [n], count) -- "group all spellings within 2 edits".
    Components chain, a null row is -1 and not counted, max_distance=None is refused, processor="default_process" as in join()."""
    edit_kind_id(measure)
    return _cluster_column(lambda c, o, v: c.distance_cluster(measure, o, v, max_distance), column, max_distance, ctx, processor,
                           cutoff="max_distance", advice="a number of edits")


__all__ = ["default_process", "PROCESSORS", "best_match", "nearest", "Codec", "Context", "device_count", "pack_strings", "split_offsets", "similarity", "levenshtein", "jaro",
           "jaro_winkler", "jaccard", "sorensen_dice", "osa", "indel", "measure_supported", "distance", "levenshtein_distance", "osa_distance",
           "indel_distance", "INDEL_MEASURES", "partial_ratio", "partial_ratio_alignment", "PARTIAL_MEASURES",
           "token_sort_ratio", "token_set_ratio", "token_sort", "TOKEN_MEASURES",
           "token_ratio", "partial_token_sort_ratio", "partial_token_set_ratio", "partial_token_ratio", "wratio", "WEIGHTED_MEASURES",
           "DISTANCE_MEASURES", "DISTANCE_UNBOUNDED", "MEASURES", "EXTRA_MEASURES", "MEASURE_ID", "STATUS", "ShapeMismatch", "StrsimError",
           "extract", "EXTRACT_SCORERS", "cdist", "CDIST_MEASURES", "join", "dedupe_pairs", "JOIN_SCORERS",
           "match_join", "match_dedupe_pairs", "MATCH_JOIN_MEASURES", "components", "cluster", "CLUSTER_MEASURES",
           "COMMON_KINDS", "hamming", "hamming_distance", "hamming_similarity", "lcs_seq", "lcs_seq_distance", "lcs_seq_similarity",
           "prefix", "prefix_distance", "prefix_similarity", "postfix", "postfix_distance", "postfix_similarity",
           "damerau_levenshtein", "damerau_levenshtein_distance", "qgram", "QGRAM_KINDS", "QGRAM_MAX_Q", "qgram_join", "qgram_dedupe_pairs", "qgram_cluster",
           "distance_join", "distance_dedupe_pairs", "distance_cluster", "DISTANCE_JOIN_MEASURES"]
