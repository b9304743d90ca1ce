"""damerau_levenshtein / damerau_levenshtein_distance through a REAL Polars engine, beside what tests/test_polars_wrappers.py holds
for the reference measures: the wrappers build expressions, and on the GPU the columns equal tests/damerau_ref.py with nulls in ->
nulls out, a literal on either side and max_distance.  Skips where Polars is not installed."""
import numpy as np
import pytest

pl = pytest.importorskip("polars")

import damerau_ref as R

A = ["ca", "jonh", None, "a cat", "", "é" * 63 + "xy", "abcdef"]
B = ["abc", "john", "x", "an abct", "", "é" * 63 + "yzx", None]


def test_dl_wrappers_build_expressions():
    import polars_strsim as ps
    assert "damerau_levenshtein" in ps.__all__ and "damerau_levenshtein_distance" in ps.__all__
    for args in (("a", "b"), (pl.col("a"), pl.lit("x")), (pl.lit("x"), "b")):
        assert isinstance(ps.damerau_levenshtein(*args), pl.Expr)
        assert isinstance(ps.damerau_levenshtein_distance(*args), pl.Expr)
        assert isinstance(ps.damerau_levenshtein_distance(*args, max_distance=2), pl.Expr)


@pytest.mark.gpu
def test_dl_columns_through_the_engine():
    import polars_strsim as ps
    df = pl.DataFrame({"a": A, "b": B}, schema={"a": pl.Utf8, "b": pl.Utf8})
    out = df.with_columns(s=ps.damerau_levenshtein("a", "b"), d=ps.damerau_levenshtein_distance("a", "b"),
                          d1=ps.damerau_levenshtein_distance("a", "b", max_distance=1),
                          lit=ps.damerau_levenshtein_distance(pl.lit("abc"), "a"), osa=ps.osa_distance("a", "b"))
    assert out["s"].dtype == pl.Float64 and out["d"].dtype == pl.UInt32 and out["d1"].dtype == pl.UInt32
    for i, (a, b) in enumerate(zip(A, B)):
        if a is None or b is None:
            assert out["s"][i] is None and out["d"][i] is None and out["d1"][i] is None
            continue
        d = R.distance(a, b)
        assert out["d"][i] == d and out["d1"][i] == min(d, 2) and out["osa"][i] >= d
        assert np.float64(out["s"][i]).view(np.uint64) == np.float64(R.score(a, b)).view(np.uint64)
    for i, a in enumerate(A):
        assert out["lit"][i] == (None if a is None else R.distance("abc", a))
