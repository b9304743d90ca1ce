"""The argument checks of the C ABI, call by call, without a GPU.

The distance, alignment, search (best-match, nearest, extract), cdist, transform (token_sort, default_process) and processed-scoring
entry points check their arguments before they look at the context, so a call with ctx = NULL reaches every check and, when nothing
is wrong, ends in "<entry point>: ctx is NULL".  Each wrong call below must return
the exact code and leave the exact strsim_last_error_message() recorded in tests/golden/capi_arg_checks.json.

That table was recorded from the library of the commit BEFORE the host-side call flows were folded (commit a8969f6, built in a
scratch copy, this file run as a script with STRSIM_AMD_LIB pointing at it):

    STRSIM_AMD_LIB=<that build>/libpolars_strsim_amd.so python tests/test_capi_arg_checks_cpu.py > tests/golden/capi_arg_checks.json

so the test pins the wording, the codes and the order of the checks across that refactor; it passes unchanged on both sides of it.
The entries of strsim_extract_*, strsim_cdist_*, strsim_token_sort_*, strsim_default_process_* and strsim_pairs_processed_* were added
by the same recipe from the library of commit a93f818, the commit BEFORE the column plumbing and the remaining flows of the C ABI
layer were folded; the entries recorded earlier did not change.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "capi_arg_checks.json")

LEVENSHTEIN, JARO, OSA, INDEL, TOKEN_SORT_RATIO = 0, 1, 6, 8, 14
PROCESS_DEFAULT = 1
NAN = float("nan")


def _column(rows):
    """A valid column of `rows` two-byte strings: (offsets, values) as numpy arrays."""
    return np.arange(0, 2 * rows + 1, 2, dtype=np.uint32), np.full(2 * rows + 1, 97, dtype=np.uint8)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _lib():
    import strsim_amd
    L = strsim_amd.lib()
    L.strsim_pairs_device_small.restype = C.c_int
    L.strsim_pairs_device_small.argtypes = L.strsim_pairs_device.argtypes
    return L


def _elementwise_cases(measures):
    """(case name, measure, a_rows, b_rows, out_rows, names of the pointers passed as NULL)"""
    m = measures[0]
    cases = [("unknown_measure_%d" % bad, bad, 3, 3, 3, ()) for bad in (JARO, 99, -1) if measures != (None,)]
    cases += [("measure_%d_valid" % ok, ok, 3, 3, 3, ()) for ok in measures[1:]]
    cases += [("shape_3_vs_2", m, 3, 2, 3, ()), ("shape_2_vs_3", m, 2, 3, 3, ()), ("shape_0_vs_2", m, 0, 2, 0, ()),
              ("literal_left_accepted", m, 1, 3, 3, ()), ("literal_right_accepted", m, 3, 1, 3, ()),
              ("out_rows_one_more", m, 3, 3, 4, ()), ("out_rows_one_less", m, 3, 3, 2, ()),
              ("out_rows_of_the_literal", m, 1, 3, 1, ()), ("shape_and_out_rows_wrong", m, 3, 2, 7, ())]
    cases += [("null_%s" % p, m, 3, 3, 3, (p,)) for p in ("a_off", "a_val", "b_off", "b_val", "out0", "out1")]
    cases += [("zero_rows_null_buffers", m, 0, 0, 0, ("a_off", "a_val", "b_off", "b_val", "out0", "out1")),
              ("zero_rows_literal_null_buffers", m, 0, 1, 0, ("a_off", "a_val", "b_off", "b_val", "out0", "out1")),
              ("valid", m, 3, 3, 3, ())]
    return cases


def _search_cases(measures, bad_measures, with_min_score):
    """(case name, measure, q_rows, c_rows, k, min_score, names of the pointers passed as NULL)"""
    m = measures[0]
    cases = [("unknown_measure_%d" % bad, bad, 3, 4, 1, 0.5, ()) for bad in bad_measures]
    cases += [("measure_%d_valid" % ok, ok, 3, 4, 1, 0.5, ()) for ok in measures[1:]]
    cases += [("k_0", m, 3, 4, 0, 0.5, ()), ("k_17", m, 3, 4, 17, 0.5, ()), ("k_16_valid", m, 3, 4, 16, 0.5, ()),
              ("k_0_and_unknown_measure", bad_measures[0], 3, 4, 0, 0.5, ())]
    if with_min_score:
        cases += [("min_score_nan", m, 3, 4, 1, NAN, ()), ("min_score_nan_and_k_0", m, 3, 4, 0, NAN, ())]
    cases += [("null_%s" % p, m, 3, 4, 1, 0.5, (p,)) for p in ("a_off", "a_val", "b_off", "b_val", "out0", "out1")]
    every = ("a_off", "a_val", "b_off", "b_val", "out0", "out1")
    cases += [("zero_queries_null_buffers", m, 0, 4, 1, 0.5, ("a_off", "a_val", "out0", "out1")),
              ("zero_rows_null_buffers", m, 0, 0, 1, 0.5, every),
              ("zero_candidates_null_candidate_buffers", m, 3, 0, 1, 0.5, ("b_off", "b_val")),
              ("query_and_candidate_buffers_null", m, 3, 4, 1, 0.5, every),
              ("valid", m, 3, 4, 1, 0.5, ())]
    return cases


def _cdist_cases():
    """(case name, measure, q_rows, c_rows, cutoff, out_ld - c_rows, names of the pointers passed as NULL)"""
    m = LEVENSHTEIN
    cases = [("unknown_measure_%d" % bad, bad, 3, 4, 0.5, 0, ()) for bad in (5, OSA, 99, -1)]
    cases += [("measure_%d_valid" % ok, ok, 3, 4, 0.5, 0, ()) for ok in (1, 2, 3, 4, INDEL, TOKEN_SORT_RATIO)]
    cases += [("cutoff_nan", m, 3, 4, NAN, 0, ()), ("cutoff_nan_and_unknown_measure", 99, 3, 4, NAN, 0, ()),
              ("out_ld_one_less", m, 3, 4, 0.5, -1, ()), ("out_ld_equal_valid", m, 3, 4, 0.5, 0, ()), ("out_ld_greater_valid", m, 3, 4, 0.5, 3, ()),
              ("out_ld_one_less_and_cutoff_nan", m, 3, 4, NAN, -1, ()), ("out_ld_one_less_and_null_a_off", m, 3, 4, 0.5, -1, ("a_off",))]
    cases += [("null_%s" % p, m, 3, 4, 0.5, 0, (p,)) for p in ("a_off", "a_val", "b_off", "b_val", "out0")]
    every = ("a_off", "a_val", "b_off", "b_val", "out0")
    cases += [("zero_queries_null_buffers", m, 0, 4, 0.5, 0, ("a_off", "a_val", "out0")),
              ("zero_candidates_null_buffers", m, 3, 0, 0.5, 0, ("b_off", "b_val", "out0")),
              ("zero_rows_null_buffers", m, 0, 0, 0.5, 0, every),
              ("every_buffer_null", m, 3, 4, 0.5, 0, every),
              ("valid", m, 3, 4, 0.5, 0, ())]
    return cases


def _transform_cases():
    """(case name, rows, out_capacity - the column's bytes, names of the pointers passed as NULL); a_* is the column, out0 / out1
    are out_off / out_val.  Every entry point tests the context before the capacity (strsim_token_sort_host tests the capacity
    before it selects the device, not before the NULL test), so with ctx = NULL the capacity_* cases pin only that order: they
    end in "ctx is NULL" or at a NULL buffer.  The capacity test itself and its wording are checked on the GPU."""
    cases = [("null_%s" % p, 3, 0, (p,)) for p in ("a_off", "a_val", "out0", "out1")]
    cases += [("zero_rows", 0, 0, ()), ("zero_rows_null_values", 0, 0, ("a_val", "out1")), ("zero_rows_null_offsets", 0, 0, ("a_off",)),
              ("zero_rows_null_out_offsets", 0, 0, ("out0",)),
              ("capacity_one_byte_short", 3, -1, ()), ("capacity_one_byte_short_and_null_out_val", 3, -1, ("out1",)),
              ("capacity_exact", 3, 0, ()), ("valid", 3, 3, ())]
    return cases


def _processed_cases():
    """(case name, measure, processor, a_rows, b_rows, out_rows, names of the pointers passed as NULL)"""
    m, pr = LEVENSHTEIN, PROCESS_DEFAULT
    cases = [("unknown_processor_%d" % bad, m, bad, 3, 3, 3, ()) for bad in (0, 2, -1)]
    cases += [("unknown_measure_%d" % bad, bad, pr, 3, 3, 3, ()) for bad in (5, 99, -1)]
    cases += [("measure_%d_valid" % ok, ok, pr, 3, 3, 3, ()) for ok in (JARO, OSA, INDEL, TOKEN_SORT_RATIO)]
    cases += [("unknown_processor_and_unknown_measure", 99, 0, 3, 3, 3, ()), ("unknown_measure_and_shape", 99, pr, 3, 2, 3, ())]
    cases += [(case, m, pr, ar, br, outr, null) for case, _, ar, br, outr, null in _elementwise_cases((m,))
              if not case.startswith("unknown_measure") and not ("out1" in null and len(null) == 1)]
    return cases


def _buffers(a_rows, b_rows, null):
    ao, av = _column(a_rows)
    bo, bv = _column(b_rows)
    out0, out1 = np.zeros(4096, dtype=np.uint64), np.zeros(4096, dtype=np.uint64)
    keep = dict(a_off=ao, a_val=av, b_off=bo, b_val=bv, out0=out0, out1=out1)
    return keep, {k: (None if k in null else _ptr(v)) for k, v in keep.items()}


def calls():
    """-> {"<entry point>/<case>": a function of the library that makes the call with ctx = NULL and returns its code}"""
    table = {}

    def add(entry, case, fn):
        assert entry + "/" + case not in table
        table[entry + "/" + case] = fn

    for suffix in ("device", "host"):
        entry = "strsim_distance_" + suffix
        for case, m, ar, br, outr, null in _elementwise_cases((LEVENSHTEIN, OSA, INDEL)):
            if "out1" in null and len(null) == 1:
                continue  # (one output)
            def fn(L, entry=entry, m=m, ar=ar, br=br, outr=outr, null=null):
                keep, p = _buffers(ar, br, null)
                return getattr(L, entry)(None, m, p["a_off"], p["a_val"], ar, p["b_off"], p["b_val"], br, 2, p["out0"], outr)
            add(entry, case, fn)
        entry = "strsim_partial_alignment_" + suffix
        for case, m, ar, br, outr, null in _elementwise_cases((None,)):
            def fn(L, entry=entry, ar=ar, br=br, outr=outr, null=null):
                keep, p = _buffers(ar, br, null)
                return getattr(L, entry)(None, p["a_off"], p["a_val"], ar, p["b_off"], p["b_val"], br, p["out0"], p["out1"], outr)
            add(entry, case, fn)
        entry = "strsim_best_match_" + suffix
        for case, m, qr, cr, k, ms, null in _search_cases((LEVENSHTEIN, 1, 2, 3, 4), (OSA, INDEL, 5, 99, -1), True):
            def fn(L, entry=entry, m=m, qr=qr, cr=cr, k=k, ms=ms, null=null):
                keep, p = _buffers(qr, cr, null)
                return getattr(L, entry)(None, m, p["a_off"], p["a_val"], qr, p["b_off"], p["b_val"], cr, k, ms, p["out0"], p["out1"])
            add(entry, case, fn)
        entry = "strsim_nearest_" + suffix
        for case, m, qr, cr, k, ms, null in _search_cases((LEVENSHTEIN, OSA), (JARO, INDEL, 99, -1), False):
            def fn(L, entry=entry, m=m, qr=qr, cr=cr, k=k, null=null):
                keep, p = _buffers(qr, cr, null)
                return getattr(L, entry)(None, m, p["a_off"], p["a_val"], qr, p["b_off"], p["b_val"], cr, k, 2, p["out0"], p["out1"])
            add(entry, case, fn)
        entry = "strsim_extract_" + suffix
        extract = _search_cases((INDEL, TOKEN_SORT_RATIO), (LEVENSHTEIN, OSA, 99, -1), True)
        extract += [("min_score_nan_and_unknown_measure", 99, 3, 4, 1, NAN, ()), ("min_score_nan_k_0_and_unknown_measure", 99, 3, 4, 0, NAN, ())]
        for case, m, qr, cr, k, cut, null in extract:  # (min_score: the score_cutoff)
            def fn(L, entry=entry, m=m, qr=qr, cr=cr, k=k, cut=cut, null=null):
                keep, p = _buffers(qr, cr, null)
                return getattr(L, entry)(None, m, p["a_off"], p["a_val"], qr, p["b_off"], p["b_val"], cr, k, cut, p["out0"], p["out1"])
            add(entry, case, fn)
        entry = "strsim_cdist_" + suffix
        for case, m, qr, cr, cut, ld, null in _cdist_cases():
            def fn(L, entry=entry, m=m, qr=qr, cr=cr, cut=cut, ld=ld, null=null):
                keep, p = _buffers(qr, cr, null)
                return getattr(L, entry)(None, m, p["a_off"], p["a_val"], qr, p["b_off"], p["b_val"], cr, cut, p["out0"], cr + ld)
            add(entry, case, fn)
        for family in ("strsim_token_sort_", "strsim_default_process_"):
            entry = family + suffix
            for case, rows, room, null in _transform_cases():
                def fn(L, entry=entry, rows=rows, room=room, null=null):
                    keep, p = _buffers(rows, 0, null)
                    return getattr(L, entry)(None, p["a_off"], p["a_val"], rows, p["out0"], p["out1"], 2 * rows + room)
                add(entry, case, fn)
        entry = "strsim_pairs_processed_" + suffix
        for case, m, pr, ar, br, outr, null in _processed_cases():
            def fn(L, entry=entry, m=m, pr=pr, ar=ar, br=br, outr=outr, null=null):
                keep, p = _buffers(ar, br, null)
                return getattr(L, entry)(None, m, pr, p["a_off"], p["a_val"], ar, p["b_off"], p["b_val"], br, p["out0"], outr)
            add(entry, case, fn)
    # the pairwise family looks at the context first
    for entry in ("strsim_pairs_device", "strsim_pairs_device_small", "strsim_pairs_host"):
        for case, m, ar, br, outr in (("valid", LEVENSHTEIN, 3, 3, 3), ("shape_3_vs_2", LEVENSHTEIN, 3, 2, 3), ("unknown_measure", 99, 3, 3, 3),
                                      ("fused_measure_id", 5, 3, 3, 3), ("zero_rows", LEVENSHTEIN, 0, 0, 0)):
            def fn(L, entry=entry, m=m, ar=ar, br=br, outr=outr):
                keep, p = _buffers(ar, br, ())
                return getattr(L, entry)(None, m, p["a_off"], p["a_val"], ar, p["b_off"], p["b_val"], br, p["out0"], outr)
            add(entry, case, fn)
    for case, ar, br, outr in (("valid", 3, 3, 3), ("shape_3_vs_2", 3, 2, 3), ("zero_rows", 0, 0, 0)):
        def fn(L, ar=ar, br=br, outr=outr):
            keep, p = _buffers(ar, br, ())
            outs = (C.c_void_p * 5)(*[p["out0"]] * 5)
            return L.strsim_pairs_device_all(None, p["a_off"], p["a_val"], ar, p["b_off"], p["b_val"], br, outs, outr)
        add("strsim_pairs_device_all", case, fn)
    return table


def observe(L, fn):
    rc = fn(L)
    return [rc, L.strsim_last_error_message().decode("utf-8") if rc else ""]


CALLS = calls()


def test_the_table_covers_every_call():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(CALLS)
    # every family is there with both forms, and the accepted calls do end at the context check
    for entry in ("strsim_distance_", "strsim_partial_alignment_", "strsim_best_match_", "strsim_nearest_", "strsim_extract_", "strsim_cdist_",
                  "strsim_pairs_processed_"):
        for suffix in ("device", "host"):
            for case in ("valid", "zero_rows_null_buffers"):
                assert golden["%s%s/%s" % (entry, suffix, case)] == [2, "%s%s: ctx is NULL" % (entry, suffix)]
    for entry in ("strsim_token_sort_", "strsim_default_process_"):
        for suffix in ("device", "host"):
            for case in ("valid", "zero_rows"):
                assert golden["%s%s/%s" % (entry, suffix, case)] == [2, "%s%s: ctx is NULL" % (entry, suffix)]
    assert golden["strsim_cdist_host/out_ld_one_less"] == [2, "strsim_cdist_host: out_ld=3 is less than the 4 candidates of a row"]
    assert golden["strsim_cdist_device/cutoff_nan_and_unknown_measure"][1].startswith("strsim_cdist_device: measure 99 is not a measure of cdist")
    assert golden["strsim_extract_device/min_score_nan_and_k_0"] == [2, "strsim_extract_device: score_cutoff is NaN"]
    assert golden["strsim_pairs_processed_host/unknown_processor_and_unknown_measure"][1].startswith("strsim_pairs_processed_host: unknown processor 0")
    assert golden["strsim_distance_device/unknown_measure_1"] == [
        2, "strsim_distance_device: measure 1 has no distance (STRSIM_LEVENSHTEIN, STRSIM_OSA or STRSIM_INDEL)"]
    assert golden["strsim_distance_host/shape_3_vs_2"] == [1, "Inputs must have the same length, or one of them must be a Utf8 literal."]
    assert golden["strsim_nearest_host/k_0"] == [2, "strsim_nearest_host: k=0 is outside 1..16"]
    assert golden["strsim_pairs_host/shape_3_vs_2"] == [2, "strsim_pairs_host: ctx is NULL"]


@pytest.mark.parametrize("key", sorted(CALLS))
def test_wrong_call_returns_the_recorded_code_and_message(key):
    golden = json.load(open(GOLDEN))
    assert observe(_lib(), CALLS[key]) == golden[key]


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "polars-strsim_amd"))
    lib_ = _lib()
    json.dump({key: observe(lib_, CALLS[key]) for key in sorted(CALLS)}, sys.stdout, indent=0, ensure_ascii=True)
    sys.stdout.write("\n")
