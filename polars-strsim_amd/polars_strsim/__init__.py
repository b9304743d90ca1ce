"""polars_strsim -- drop-in package directory for the MI355X build.

Same five expression functions, signatures and `is_elementwise=True` registration as the reference
(reference polars_strsim/__init__.py:8-69).  Polars resolves the plugin by scanning this directory for a
shared library, finds libpolars_strsim_amd.so (built here by ../Makefile) and calls its
`_polars_plugin_<name>` symbols (include/polars_plugin_abi.h), which run on the GPU.
"""
import ctypes as _C
import importlib.util as _ilu
import os as _os
import sys as _sys
from pathlib import Path

import polars as pl
from polars._typing import IntoExpr
from polars.plugins import register_plugin_function

from polars_strsim.utils import parse_into_expr

_PLUGIN_DIR = Path(__file__).parent


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process (the same rule as strsim_amd/_lib.py, for the route where POLARS loads the library).

    Polars dlopen()s libpolars_strsim_amd.so on the first plugin call; it then binds /opt/rocm's libamdhip64.  A torch wheel
    brings its own copy, and an `import torch` AFTER that maps the second runtime next to the first -- whichever initialises
    second finds "No HIP GPUs".  When torch is installed but not imported yet, its copy is mapped first (by SONAME both
    then resolve to it); when torch is already imported nothing needs doing; without torch the system runtime is used.
    Set STRSIM_KEEP_SYSTEM_HIP=1 to switch this off."""
    if "torch" in _sys.modules or _os.environ.get("STRSIM_KEEP_SYSTEM_HIP"):
        return
    try:
        spec = _ilu.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    bundled = _os.path.join(_os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if _os.path.exists(bundled):
        _C.CDLL(bundled, mode=_C.RTLD_GLOBAL)


_share_hip_runtime_with_torch()


def _similarity(function_name: str, expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name=function_name,
        args=[parse_into_expr(expr, dtype=pl.Utf8), parse_into_expr(other, dtype=pl.Utf8)],
        is_elementwise=True,
    )


def levenshtein(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Normalised Levenshtein similarity of two string columns (or a column and a literal)."""
    return _similarity("levenshtein", expr, other)


def jaro(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Jaro similarity."""
    return _similarity("jaro", expr, other)


def jaro_winkler(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Jaro-Winkler similarity (prefix scale 0.1, prefix cap 4, boost threshold 0.7)."""
    return _similarity("jaro_winkler", expr, other)


def jaccard(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Jaccard similarity of the two character multisets."""
    return _similarity("jaccard", expr, other)


def sorensen_dice(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Sorensen-Dice similarity of the two character multisets."""
    return _similarity("sorensen_dice", expr, other)


def osa(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Optimal string alignment: the restricted Damerau-Levenshtein (OSA) similarity.

    Levenshtein with one more edit: a swap of two adjacent characters costs 1 ("jonh" / "john" is 0.75, not 0.5).  Restricted:
    no substring is edited twice, so ("ca", "abc") is 3 edits, where the unrestricted Damerau-Levenshtein distance (`damerau_levenshtein`) is 2.
    Normalised like levenshtein: 1 - distance / max(len), over characters; 1.0 when both strings are empty.  Not a measure of
    the upstream polars-strsim.
    """
    return _similarity("osa", expr, other)


def indel(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Indel similarity: rapidfuzz `fuzz.ratio` / 100 (`Indel.normalized_similarity`).

    With l the length of the longest common subsequence, the distance is len(a) + len(b) - 2 l: insertions and deletions only,
    so a substitution costs 2 ("ab" / "ba" is 0.5).  The score is 1 - distance / (len(a) + len(b)) over characters, 1.0 when
    both strings are empty.  Not a measure of the upstream polars-strsim.
    """
    return _similarity("indel", expr, other)


def partial_ratio(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Partial ratio: rapidfuzz `fuzz.partial_ratio` / 100.

    The best `indel` score of the shorter string (the needle, m characters) against a window of the longer one.  The windows are
    the longer string's proper prefixes of 1 .. m-1 characters, every substring of m characters, and its proper suffixes: the
    needle slid over it one step at a time, overhanging either end.  For equal lengths the larger of the two directions; 1.0 when
    both strings are empty, 0.0 when exactly one is.  It can be lower than `indel` of the same pair: when the lengths differ the
    whole longer string is not one of the windows.  It is the maximum at every needle length (rapidfuzz switches to a heuristic
    for needles of more than 64 characters; this does not).  Not in the upstream polars-strsim.
    """
    return _similarity("partial_ratio", expr, other)


def partial_ratio_alignment(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """`partial_ratio` with the window that won (rapidfuzz `fuzz.partial_ratio` / 100 and `fuzz.partial_ratio_alignment`): a
    struct {score: Float64, src_start, src_end, dest_start, dest_end: UInt32}; src is `expr`, dest is `other`, spans are half
    open and counted in characters.  The needle (the shorter string) spans (0, its length), the other span is the winning window
    out of the window set of `partial_ratio`; among windows with the same score the one with the smallest end wins, then the
    smallest start.  Null in, null out.  Not in the upstream polars-strsim."""
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="partial_ratio_alignment",
        args=[parse_into_expr(expr), other],
        is_elementwise=True,
    )


def token_sort_ratio(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """rapidfuzz `fuzz.token_sort_ratio` / 100: `indel` of the two strings with their tokens sorted.

    Tokens are split at whitespace -- exactly Python's `str.isspace` set, 29 code points, as `str.split()` does -- sorted by code
    point (a proper prefix first) and joined with one space; duplicates are kept.  `"smith john"` and `"john  smith"` score 1.0.
    Two strings without tokens give 1.0, exactly one gives 0.0.  No lower-casing or other pre-processing.
    Not in the upstream polars-strsim.
    """
    return _similarity("token_sort_ratio", expr, other)


def token_set_ratio(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """rapidfuzz `fuzz.token_set_ratio` / 100 over the sets of tokens (split at Python's `str.isspace` set, as
    `token_sort_ratio`): 0.0 when either string has no token; 1.0 when the sets share a token and one contains the other; else
    the best `indel` among the pairs of sect, sect + " " + ab and sect + " " + ba (the joined sorted intersection and the two
    differences).  Not in the upstream polars-strsim."""
    return _similarity("token_set_ratio", expr, other)


def token_ratio(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """rapidfuzz `fuzz.token_ratio` / 100: the larger of `token_sort_ratio` and `token_set_ratio` of the pair.
    Not in the upstream polars-strsim."""
    return _similarity("token_ratio", expr, other)


def partial_token_sort_ratio(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """rapidfuzz `fuzz.partial_token_sort_ratio` / 100: `partial_ratio` of the two strings with their tokens sorted (split, sorted
    and joined as for `token_sort_ratio`).  Not in the upstream polars-strsim."""
    return _similarity("partial_token_sort_ratio", expr, other)


def partial_token_set_ratio(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """rapidfuzz `fuzz.partial_token_set_ratio` / 100 over the sets of tokens: 0.0 when either string has no token, 1.0 when the
    sets share a token, else `partial_ratio` of the two joined sorted differences.  Not in the upstream polars-strsim."""
    return _similarity("partial_token_set_ratio", expr, other)


def partial_token_ratio(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """rapidfuzz `fuzz.partial_token_ratio` / 100: the larger of `partial_token_sort_ratio` and `partial_token_set_ratio`.
    Not in the upstream polars-strsim."""
    return _similarity("partial_token_ratio", expr, other)


def wratio(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """rapidfuzz `fuzz.WRatio` / 100, the default scorer of `process.extract`, without a processor (no lower-casing).

    With lo and hi the shorter and the longer length in characters and r = `indel`: 0.0 when a string is empty; when
    2 hi < 3 lo, max(r, `token_ratio` * 0.95); otherwise max(r, `partial_ratio` * ps, `partial_token_ratio` * 0.95 * ps) with
    ps = 0.9 when hi <= 8 lo and 0.6 beyond.  `"this is a test"` against `"this is a new test!!!"` scores 0.855.  The GPU sorts
    the rows into the two classes first and runs each family of scores over its own rows only.
    Not in the upstream polars-strsim.
    """
    return _similarity("wratio", expr, other)


def _distance(function_name: str, expr: IntoExpr, other: IntoExpr, max_distance: int | None) -> pl.Expr:
    args = [parse_into_expr(expr), other]
    if max_distance is not None:
        args.append(pl.lit(max_distance, dtype=pl.UInt32))
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name=function_name,
        args=args,
        is_elementwise=True,
    )


def levenshtein_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:
    """Levenshtein distance (insert, delete, substitute, each 1) over characters, as UInt32.

    With max_distance=k a row is the distance when it is at most k and k + 1 otherwise (rapidfuzz's score_cutoff), which the GPU
    decides early: `levenshtein_distance(a, b, max_distance=2) <= 2` is "at most two typos".  Not in the upstream polars-strsim.
    """
    return _distance("levenshtein_distance", expr, other, max_distance)


def osa_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:
    """Optimal string alignment distance: levenshtein_distance plus a swap of two adjacent characters costing 1, no substring
    edited twice.  max_distance as in levenshtein_distance.  Not in the upstream polars-strsim."""
    return _distance("osa_distance", expr, other, max_distance)


def indel_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:
    """Indel distance as UInt32: len(a) + len(b) - 2 LCS(a, b) over characters -- insertions and deletions only, a substitution
    costs 2.  `indel` (rapidfuzz `fuzz.ratio` / 100) is 1 - indel_distance / (len(a) + len(b)).  max_distance as in
    levenshtein_distance.  Not in the upstream polars-strsim."""
    return _distance("indel_distance", expr, other, max_distance)


def damerau_levenshtein(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Unrestricted Damerau-Levenshtein similarity (strsim's `normalized_damerau_levenshtein`, rapidfuzz's
    `DamerauLevenshtein.normalized_similarity`).

    Like `osa`, a swap of two adjacent characters costs 1; unlike it, a substring may be edited again after a swap, so
    ("ca", "abc") is 2 edits, not 3, and the distance is a metric.  Normalised like levenshtein: 1 - distance / max(len), over
    characters; 1.0 when both strings are empty.  A cell DP on the GPU, slower than `osa`.  Not in the upstream polars-strsim.
    """
    return _similarity("damerau_levenshtein", expr, other)


def damerau_levenshtein_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:
    """Unrestricted Damerau-Levenshtein distance as UInt32 (see damerau_levenshtein); never more than osa_distance.
    max_distance as in levenshtein_distance.  Not in the upstream polars-strsim."""
    return _distance("damerau_levenshtein_distance", expr, other, max_distance)


def hamming(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Normalised Hamming similarity (rapidfuzz's `Hamming.normalized_similarity`): 1 - hamming_distance / max(len) over
    characters, 1.0 when both strings are empty.  Strings of different lengths are padded: the difference of the lengths counts
    as mismatches.  To have nulls there instead, compose:
    `pl.when(a.str.len_chars() == b.str.len_chars()).then(hamming(a, b))`.  Not in the upstream polars-strsim."""
    return _similarity("hamming", expr, other)


def hamming_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:
    """Hamming distance as UInt32 (strsim's `hamming`, DuckDB's `hamming` / `mismatches`): the positions at which the two strings
    differ, over characters, plus the difference of their lengths (rapidfuzz's pad=True).  For equal lengths only:
    `pl.when(a.str.len_chars() == b.str.len_chars()).then(hamming_distance(a, b))`.  max_distance as in levenshtein_distance.
    Not in the upstream polars-strsim."""
    return _distance("hamming_distance", expr, other, max_distance)


def hamming_similarity(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """The positions at which the two strings agree, as UInt32 (rapidfuzz's `Hamming.similarity`).  Not in the upstream polars-strsim."""
    return _distance("hamming_similarity", expr, other, None)


def lcs_seq(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Normalised LCSseq similarity (rapidfuzz's `LCSseq.normalized_similarity`): the length of the longest common subsequence over
    characters, divided by max(len); 1.0 when both strings are empty.  Not `indel`, which divides twice that length by the sum of
    the lengths.  Not in the upstream polars-strsim."""
    return _similarity("lcs_seq", expr, other)


def lcs_seq_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:
    """max(len) minus the length of the longest common subsequence, as UInt32 (rapidfuzz's `LCSseq.distance`).  max_distance as in
    levenshtein_distance.  Not in the upstream polars-strsim."""
    return _distance("lcs_seq_distance", expr, other, max_distance)


def lcs_seq_similarity(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """The length of the longest common subsequence over characters, as UInt32 (rapidfuzz's `LCSseq.similarity`).  Not in the
    upstream polars-strsim."""
    return _distance("lcs_seq_similarity", expr, other, None)


def prefix(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Normalised common-prefix similarity (rapidfuzz's `Prefix.normalized_similarity`): the length of the longest common prefix
    over characters, divided by max(len); 1.0 when both strings are empty.  Not in the upstream polars-strsim."""
    return _similarity("prefix", expr, other)


def prefix_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:
    """max(len) minus the length of the longest common prefix, as UInt32 (rapidfuzz's `Prefix.distance`).  max_distance as in
    levenshtein_distance.  Not in the upstream polars-strsim."""
    return _distance("prefix_distance", expr, other, max_distance)


def prefix_similarity(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """The length of the longest common prefix over characters, as UInt32 (rapidfuzz's `Prefix.similarity`).  Not in the upstream
    polars-strsim."""
    return _distance("prefix_similarity", expr, other, None)


def postfix(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """Normalised common-suffix similarity (rapidfuzz's `Postfix.normalized_similarity`): the length of the longest common suffix
    over characters, divided by max(len); 1.0 when both strings are empty.  Not in the upstream polars-strsim."""
    return _similarity("postfix", expr, other)


def postfix_distance(expr: IntoExpr, other: IntoExpr, max_distance: int | None = None) -> pl.Expr:
    """max(len) minus the length of the longest common suffix, as UInt32 (rapidfuzz's `Postfix.distance`).  max_distance as in
    levenshtein_distance.  Not in the upstream polars-strsim."""
    return _distance("postfix_distance", expr, other, max_distance)


def postfix_similarity(expr: IntoExpr, other: IntoExpr) -> pl.Expr:
    """The length of the longest common suffix over characters, as UInt32 (rapidfuzz's `Postfix.similarity`).  Not in the upstream
    polars-strsim."""
    return _distance("postfix_similarity", expr, other, None)


def default_process(expr: IntoExpr) -> pl.Expr:
    """rapidfuzz `utils.default_process` on the GPU, String in and String out: every character that is neither alphanumeric nor
    "_" becomes a space, the others are lower-cased, and spaces are removed from both ends (inner runs of spaces stay:
    "Apple, Inc." -> "apple  inc").  `indel(default_process(a), default_process(b))` is rapidfuzz's
    `fuzz.ratio(a, b, processor=utils.default_process)` / 100.  Character by character: U+03A3 is lower-cased to U+03C3 in every
    position and U+0130 to "i".  Nulls stay null.  Not in the upstream polars-strsim."""
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="default_process",
        args=[parse_into_expr(expr, dtype=pl.Utf8)],
        is_elementwise=True,
    )


__all__ = [
    "default_process",
    "best_match",
    "nearest",
    "levenshtein_distance",
    "osa_distance",
    "osa",
    "damerau_levenshtein_distance",
    "damerau_levenshtein",
    "hamming", "hamming_distance", "hamming_similarity",
    "lcs_seq", "lcs_seq_distance", "lcs_seq_similarity",
    "prefix", "prefix_distance", "prefix_similarity",
    "postfix", "postfix_distance", "postfix_similarity",
    "indel_distance",
    "indel",
    "partial_ratio",
    "partial_ratio_alignment",
    "token_sort_ratio",
    "token_set_ratio",
    "token_ratio",
    "partial_token_sort_ratio",
    "partial_token_set_ratio",
    "partial_token_ratio",
    "wratio",
    "levenshtein",
    "jaro",
    "jaro_winkler",
    "jaccard",
    "sorensen_dice",
    "extract",
]


_BEST_MATCH_MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")


def best_match(expr: IntoExpr, candidates: IntoExpr, measure: str = "jaro_winkler") -> pl.Expr:
    """The best candidate of every row of `expr` among all rows of `candidates` (any length), by `measure`: a struct
    {index: UInt32, score: Float64}, null where the row is null or no candidate is; ties go to the lower candidate index."""
    if measure not in _BEST_MATCH_MEASURES:
        raise ValueError(f"unknown measure {measure!r}; expected one of {_BEST_MATCH_MEASURES}")
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="best_match_" + measure,
        args=[parse_into_expr(expr, dtype=pl.Utf8), parse_into_expr(candidates, dtype=pl.Utf8)],
        is_elementwise=False,
    )


_NEAREST_MEASURES = ("levenshtein", "osa")


def nearest(expr: IntoExpr, candidates: IntoExpr, measure: str = "levenshtein", max_distance: int | None = None) -> pl.Expr:
    """The nearest candidate of every row of `expr` among all rows of `candidates` (any length) by edit distance ("levenshtein"
    or "osa"): a struct {index: UInt32, distance: UInt32}, null where the row is null or no candidate is within max_distance
    (None: no cutoff); ties go to the lower candidate index.  rapidfuzz's process.extractOne with a distance scorer and
    score_cutoff.  Not in the upstream polars-strsim."""
    if measure not in _NEAREST_MEASURES:
        raise ValueError(f"unknown measure {measure!r}; expected one of {_NEAREST_MEASURES}")
    args = [parse_into_expr(expr, dtype=pl.Utf8), parse_into_expr(candidates, dtype=pl.Utf8)]
    if max_distance is not None:
        args.append(pl.lit(max_distance, dtype=pl.UInt32))
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="nearest_" + measure,
        args=args,
        is_elementwise=False,
    )


_EXTRACT_SCORERS = ("ratio", "token_sort_ratio")


def extract(expr: IntoExpr, candidates: IntoExpr, scorer: str = "ratio", score_cutoff: float | None = None) -> pl.Expr:
    """The best candidate of every row of `expr` among all rows of `candidates` (any length) by `scorer` ("ratio" or
    "token_sort_ratio"): a struct {index: UInt32, score: Float64}, null where the row is null or no candidate scores at least
    score_cutoff (None: no cutoff); ties go to the lower candidate index.  rapidfuzz's process.extractOne with fuzz.ratio or
    fuzz.token_sort_ratio as the scorer; the score is theirs / 100, in [0, 1], and so is score_cutoff.  Not in the upstream
    polars-strsim."""
    if scorer not in _EXTRACT_SCORERS:
        raise ValueError(f"unknown scorer {scorer!r}; expected one of {_EXTRACT_SCORERS}")
    args = [parse_into_expr(expr, dtype=pl.Utf8), parse_into_expr(candidates, dtype=pl.Utf8)]
    if score_cutoff is not None:
        args.append(pl.lit(score_cutoff, dtype=pl.Float64))
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="extract_" + scorer,
        args=args,
        is_elementwise=False,
    )


# (a statement of its own: the list above closes with "extract")
__all__ += ["cdist"]

_CDIST_MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice", "ratio", "token_sort_ratio")


def cdist(expr: IntoExpr, candidates: IntoExpr, measure: str = "ratio", score_cutoff: float | None = None) -> pl.Expr:
    """The scores of every row of `expr` against all rows of `candidates` (any length M) by `measure` (one of the five reference
    measures, "ratio" or "token_sort_ratio"): a List(Float64) of M scores per row, in the order of `candidates`; a score below
    score_cutoff is 0.0 (None: no cutoff).  A null row gives a null list and a null candidate a null element.  rapidfuzz's
    process.cdist, row by row; for "ratio" and "token_sort_ratio" the score is fuzz.ratio / fuzz.token_sort_ratio / 100, in [0, 1],
    and so is score_cutoff.  Not in the upstream polars-strsim."""
    if measure not in _CDIST_MEASURES:
        raise ValueError(f"unknown measure {measure!r}; expected one of {_CDIST_MEASURES}")
    args = [parse_into_expr(expr, dtype=pl.Utf8), parse_into_expr(candidates, dtype=pl.Utf8)]
    if score_cutoff is not None:
        args.append(pl.lit(score_cutoff, dtype=pl.Float64))
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="cdist_" + measure,
        args=args,
        is_elementwise=False,
    )


# (a statement of its own again)
__all__ += ["join"]

_JOIN_SCORERS = ("ratio", "token_sort_ratio")


def join(expr: IntoExpr, candidates: IntoExpr, scorer: str = "ratio", score_cutoff: float | None = None) -> pl.Expr:
    """Every row of `candidates` (any length) that scores at least score_cutoff against the row of `expr`, by `scorer` ("ratio" or
    "token_sort_ratio"): a List(Struct{index: UInt32, score: Float64}) per row, in ascending candidate index, nothing truncated (a
    name with 40 duplicates lists all 40); None reports every candidate.  A null row gives a null list, a row without a hit an empty
    one; null candidates are never matched.  The score is fuzz.ratio / fuzz.token_sort_ratio / 100, in [0, 1], and so is
    score_cutoff.  Not in the upstream polars-strsim."""
    if scorer not in _JOIN_SCORERS:
        raise ValueError(f"unknown scorer {scorer!r}; expected one of {_JOIN_SCORERS}")
    args = [parse_into_expr(expr, dtype=pl.Utf8), parse_into_expr(candidates, dtype=pl.Utf8)]
    if score_cutoff is not None:
        args.append(pl.lit(score_cutoff, dtype=pl.Float64))
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="join_" + scorer,
        args=args,
        is_elementwise=False,
    )


# (a statement of its own again)
__all__ += ["match_join"]

_MATCH_JOIN_MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")


def match_join(expr: IntoExpr, candidates: IntoExpr, measure: str = "jaro_winkler", min_score: float | None = None) -> pl.Expr:
    """Every row of `candidates` (any length) that scores at least min_score against the row of `expr`, by `measure` (one of the
    five measures of this package): a List(Struct{index: UInt32, score: Float64}) per row, in ascending candidate index, nothing
    truncated; None reports every candidate.  A null row gives a null list, a row without a hit an empty one; null candidates are
    never matched.  The score is the pairwise function's, bit for bit.  Not in the upstream polars-strsim."""
    if measure not in _MATCH_JOIN_MEASURES:
        raise ValueError(f"unknown measure {measure!r}; expected one of {_MATCH_JOIN_MEASURES}")
    args = [parse_into_expr(expr, dtype=pl.Utf8), parse_into_expr(candidates, dtype=pl.Utf8)]
    if min_score is not None:
        args.append(pl.lit(min_score, dtype=pl.Float64))
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="match_join_" + measure,
        args=args,
        is_elementwise=False,
    )


# (a statement of its own again)
__all__ += ["cluster"]

_CLUSTER_MEASURES = _MATCH_JOIN_MEASURES + _JOIN_SCORERS


def cluster(expr: IntoExpr, measure: str = "jaro_winkler", min_score: float | None = None) -> pl.Expr:
    """The duplicate groups of a column: rows that score at least min_score by `measure` (one of the five measures of this package,
    "ratio" or "token_sort_ratio") are linked, and every row gets the row number of the first member of its group, as UInt32 --

        df.with_columns(g=cluster("name", "jaro_winkler", 0.92)).group_by("g")

    groups the spellings of one customer.  Groups are the connected components of the links, so they chain: a~b~c puts `a` and `c`
    together even where they do not match each other.  A null row gives null and never joins anything.  min_score is required (None
    would put every row in one group).  The whole column is clustered at once, whatever its chunks.  Not in the upstream
    polars-strsim."""
    if measure not in _CLUSTER_MEASURES:
        raise ValueError(f"unknown measure {measure!r}; expected one of {_CLUSTER_MEASURES}")
    if min_score is None:
        raise ValueError("cluster: min_score is required (None would put every row in one group)")
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="cluster_" + measure,
        args=[parse_into_expr(expr, dtype=pl.Utf8), pl.lit(min_score, dtype=pl.Float64)],
        is_elementwise=False,
    )


# (a statement of its own again)
__all__ += ["qgram_jaccard", "qgram_sorensen_dice", "qgram_overlap", "qgram_cosine"]

_QGRAM_KINDS = ("jaccard", "sorensen_dice", "overlap", "cosine")


def _qgram_mode(kind: str, q: int, multiset: bool) -> list:
    """q and the set flag as the plugin takes them, two UInt32 literals; ValueError for an unknown kind or a q outside 1 .. 3"""
    if kind not in _QGRAM_KINDS:
        raise ValueError(f"unknown q-gram kind {kind!r}; expected one of {_QGRAM_KINDS}")
    if isinstance(q, bool) or not isinstance(q, int) or not 1 <= q <= 3:
        raise ValueError(f"q={q!r} is outside 1 .. 3")
    return [pl.lit(q, dtype=pl.UInt32), pl.lit(0 if multiset else 1, dtype=pl.UInt32)]


def _qgram(kind: str, expr: IntoExpr, other: IntoExpr, q: int, multiset: bool) -> pl.Expr:
    mode = _qgram_mode(kind, q, multiset)
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="qgram_" + kind,
        args=[parse_into_expr(expr), other] + mode,
        is_elementwise=True,
    )


def qgram_jaccard(expr: IntoExpr, other: IntoExpr, q: int = 2, multiset: bool = True) -> pl.Expr:
    """Jaccard similarity over q-grams (q consecutive characters, q = 1, 2 or 3): I / (na + nb - I), with na and nb the grams of
    the two strings and I those they share.  multiset=True counts a repeated gram as often as it occurs (I is the sum of the
    smaller counts), False compares the sets of distinct grams.  Equal strings score 1.0, also when they are shorter than q;
    otherwise a string without a gram scores 0.0.  `jaccard` is this at q = 1: there "abc" and "cba" score 1.0, here, at q = 2,
    0.0.  Not in the upstream polars-strsim."""
    return _qgram("jaccard", expr, other, q, multiset)


def qgram_sorensen_dice(expr: IntoExpr, other: IntoExpr, q: int = 2, multiset: bool = True) -> pl.Expr:
    """Sorensen-Dice similarity over q-grams: 2 I / (na + nb); q, multiset and the edge cases as in `qgram_jaccard`.  At q = 2 this
    is the bigram Dice coefficient of the Rust `strsim` crate, without its removal of whitespace; `sorensen_dice` is this at q = 1.
    Not in the upstream polars-strsim."""
    return _qgram("sorensen_dice", expr, other, q, multiset)


def qgram_overlap(expr: IntoExpr, other: IntoExpr, q: int = 2, multiset: bool = True) -> pl.Expr:
    """Overlap coefficient over q-grams: I / min(na, nb) -- 1.0 when the grams of one string are all found in the other; q,
    multiset and the edge cases as in `qgram_jaccard`.  Not in the upstream polars-strsim."""
    return _qgram("overlap", expr, other, q, multiset)


def qgram_cosine(expr: IntoExpr, other: IntoExpr, q: int = 2, multiset: bool = True) -> pl.Expr:
    """Cosine (Ochiai) coefficient over q-grams: I / sqrt(na nb); q, multiset and the edge cases as in `qgram_jaccard`.  Not in the
    upstream polars-strsim."""
    return _qgram("cosine", expr, other, q, multiset)


# (a statement of its own again)
__all__ += ["qgram_join", "qgram_cluster"]


def qgram_join(expr: IntoExpr, candidates: IntoExpr, kind: str = "sorensen_dice", q: int = 2, multiset: bool = True,
               min_score: float | None = None) -> pl.Expr:
    """Every row of `candidates` (any length) whose q-gram similarity to the row of `expr` is at least min_score -- `kind` is
    "jaccard", "sorensen_dice", "overlap" or "cosine", q and multiset as in `qgram_jaccard`: a List(Struct{index: UInt32, score:
    Float64}) per row, in ascending candidate index, nothing truncated; None reports every candidate.  A null row gives a null list,
    a row without a hit an empty one; null candidates are never matched.  The score is the pairwise qgram_<kind> function's, bit for
    bit.  Not in the upstream polars-strsim."""
    args = [parse_into_expr(expr, dtype=pl.Utf8), parse_into_expr(candidates, dtype=pl.Utf8)] + _qgram_mode(kind, q, multiset)
    if min_score is not None:
        args.append(pl.lit(min_score, dtype=pl.Float64))
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="qgram_join_" + kind,
        args=args,
        is_elementwise=False,
    )


def qgram_cluster(expr: IntoExpr, kind: str = "sorensen_dice", q: int = 2, multiset: bool = True, min_score: float | None = None) -> pl.Expr:
    """The duplicate groups of a column by q-gram similarity: `cluster` with the rows linked whose qgram_<kind> score (q and
    multiset as in `qgram_jaccard`) is at least min_score.  Every row gets the row number of the first member of its group, as
    UInt32; groups chain, a null row gives null, min_score is required.  Not in the upstream polars-strsim."""
    mode = _qgram_mode(kind, q, multiset)
    if min_score is None:
        raise ValueError("qgram_cluster: min_score is required (None would put every row in one group)")
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="qgram_cluster_" + kind,
        args=[parse_into_expr(expr, dtype=pl.Utf8)] + mode + [pl.lit(min_score, dtype=pl.Float64)],
        is_elementwise=False,
    )


# (a statement of its own again)
__all__ += ["distance_join", "distance_cluster"]

_DISTANCE_JOIN_MEASURES = ("levenshtein", "osa", "damerau_levenshtein")


def _distance_join_measure(measure: str, max_distance) -> None:
    """ValueError for an unknown measure or a max_distance that is not None or an int in 0 .. 2^32 - 2"""
    if measure not in _DISTANCE_JOIN_MEASURES:
        raise ValueError(f"unknown measure {measure!r}; expected one of {_DISTANCE_JOIN_MEASURES}")
    if max_distance is not None and (isinstance(max_distance, bool) or not isinstance(max_distance, int) or not 0 <= max_distance < 0xFFFFFFFF):
        raise ValueError(f"max_distance={max_distance!r} is not None or an int in 0 .. 2^32 - 2")


def distance_join(expr: IntoExpr, candidates: IntoExpr, measure: str = "levenshtein", max_distance: int | None = None) -> pl.Expr:
    """Every row of `candidates` (any length) within max_distance edits of the row of `expr` by `measure` ("levenshtein", "osa" or
    "damerau_levenshtein", the unrestricted distance): a List(Struct{index: UInt32, distance: UInt32}) per row, in ascending
    candidate index, nothing truncated; max_distance=0 lists the exact duplicates, None every candidate.  A null row gives a null
    list, a row without a hit an empty one; null candidates are never matched.  The distance is the pairwise
    <measure>_distance function's.  Not in the upstream polars-strsim."""
    _distance_join_measure(measure, max_distance)
    args = [parse_into_expr(expr, dtype=pl.Utf8), parse_into_expr(candidates, dtype=pl.Utf8)]
    if max_distance is not None:
        args.append(pl.lit(max_distance, dtype=pl.UInt32))
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="distance_join_" + measure,
        args=args,
        is_elementwise=False,
    )


def distance_cluster(expr: IntoExpr, measure: str = "levenshtein", max_distance: int | None = None) -> pl.Expr:
    """The duplicate groups of a column by edit distance: `cluster` with the rows linked that are within max_distance edits by
    `measure` (as in `distance_join`) -- "group all spellings within 2 edits".  Every row gets the row number of the first member
    of its group, as UInt32; groups chain, a null row gives null, max_distance is required.  Not in the upstream polars-strsim."""
    _distance_join_measure(measure, max_distance)
    if max_distance is None:
        raise ValueError("distance_cluster: max_distance is required (None would put every row in one group)")
    return register_plugin_function(
        plugin_path=_PLUGIN_DIR,
        function_name="distance_cluster_" + measure,
        args=[parse_into_expr(expr, dtype=pl.Utf8), pl.lit(max_distance, dtype=pl.UInt32)],
        is_elementwise=False,
    )
