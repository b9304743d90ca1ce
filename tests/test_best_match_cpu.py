"""Best match (ABI 1.7) without a GPU: the exported symbols and version, argument errors before any device, and the NumPy
reference top-k of the GPU tests against a brute-force sort."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import best_match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "polars-strsim_amd", "polars_strsim", "libpolars_strsim_amd.so")
ERR_ARG = 2


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    L = C.CDLL(LIB)
    vp, u64 = C.c_void_p, C.c_uint64
    for name in ("strsim_best_match_device", "strsim_best_match_host"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, u64, C.c_uint32, C.c_double, vp, vp]
    L.strsim_abi_version.restype = C.c_uint32
    L.strsim_last_error_message.restype = C.c_char_p
    return L


def test_version_is_1_7(L):
    assert L.strsim_abi_version() == 0x00010007
    hdr = open(os.path.join(ROOT, "include", "strsim_amd.h")).read()
    assert re.search(r"#define STRSIM_ABI_VERSION 0x00010007u", hdr)


def test_best_match_symbols_are_exported(L):
    for name in ("strsim_best_match_device", "strsim_best_match_host"):
        assert getattr(L, name) is not None
    PL = C.CDLL(LIB)
    for m in ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice"):
        assert getattr(PL, "_polars_plugin_best_match_" + m) is not None
        assert getattr(PL, "_polars_plugin_field_best_match_" + m) is not None


def _call(L, name, k=1, q_rows=1, c_rows=1, min_score=0.0, measure=0, null_q=False, null_out=False, null_c=False):
    qo = (C.c_uint32 * 2)(0, 1)
    qv = (C.c_uint8 * 1)(97)
    idx = (C.c_uint32 * 32)()
    sc = (C.c_double * 32)()
    f = getattr(L, name)
    return f(None, measure, None if null_q else C.addressof(qo), C.addressof(qv), q_rows, None if null_c else C.addressof(qo),
             C.addressof(qv), c_rows, k, min_score, None if null_out else C.addressof(idx), None if null_out else C.addressof(sc))


@pytest.mark.parametrize("name", ["strsim_best_match_device", "strsim_best_match_host"])
@pytest.mark.parametrize("case,kw,msg", [
    ("k0", dict(k=0), "k=0"),
    ("k17", dict(k=17), "k=17"),
    ("measure", dict(measure=5), "measure"),
    ("nan", dict(min_score=float("nan")), "NaN"),
    ("null_queries", dict(null_q=True), "NULL"),
    ("null_outputs", dict(null_out=True), "NULL"),
    ("null_candidates", dict(null_c=True), "NULL"),
    ("too_many_candidates", dict(c_rows=2 ** 32 - 1), "candidates"),
])
def test_argument_errors_need_no_device(L, name, case, kw, msg):
    # the arguments are checked before the context: STRSIM_ERR_ARG, with the reason in the message, on a box without a GPU
    assert _call(L, name, **kw) == ERR_ARG
    assert msg in L.strsim_last_error_message().decode()


@pytest.mark.parametrize("name", ["strsim_best_match_device", "strsim_best_match_host"])
def test_null_context_is_an_argument_error(L, name):
    assert _call(L, name, k=16) == ERR_ARG
    assert "ctx is NULL" in L.strsim_last_error_message().decode()


@pytest.mark.parametrize("seed", range(6))
def test_reference_topk_matches_a_brute_force_sort(seed):
    rng = np.random.default_rng(seed)
    n, m = 7, int(rng.integers(0, 40))
    scores = rng.integers(0, 5, size=(n, m)).astype(np.float64) / 4.0  # many ties
    for k in (1, 3, 16):
        for ms in (None, 0.5, 0.51, 1.0):
            a = R.topk(scores, k, ms)
            b = R.brute_topk(scores, k, ms)
            assert np.array_equal(a[0], b[0])
            assert np.array_equal(a[1], b[1], equal_nan=True)


def test_reference_topk_tie_rule():
    s = np.array([[0.5, 0.9, 0.5, 0.9, 0.1]])
    idx, val = R.topk(s, 4)
    assert idx.tolist() == [[1, 3, 0, 2]]
    idx, val = R.topk(s, 7, 0.5)
    assert idx.tolist() == [[1, 3, 0, 2, -1, -1, -1]]
    assert np.isnan(val[0, 4:]).all()
