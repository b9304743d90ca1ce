"""polars_strsim.partial_ratio / partial_ratio_alignment through a REAL Polars engine.  Polars is not in every image: without it
this file skips."""
import inspect

import numpy as np
import pytest

pl = pytest.importorskip("polars")

import partial_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_partial_wrapper_signatures_and_all():
    import polars_strsim as ps
    assert "partial_ratio" in ps.__all__ and "partial_ratio_alignment" in ps.__all__
    for f in (ps.partial_ratio, ps.partial_ratio_alignment):
        assert list(inspect.signature(f).parameters) == ["expr", "other"]
        assert "fuzz.partial_ratio" in f.__doc__ and "/ 100" in f.__doc__ and "upstream polars-strsim" in f.__doc__
    for args in (("a", "b"), (pl.col("a"), pl.lit("x")), (pl.lit("x"), "b")):
        assert isinstance(ps.partial_ratio(*args), pl.Expr) and isinstance(ps.partial_ratio_alignment(*args), pl.Expr)
    with pytest.raises(ValueError):
        ps.best_match("a", "b", measure="partial_ratio")
    with pytest.raises(ValueError):
        ps.nearest("a", "b", measure="partial_ratio")


def test_partial_ratio_column_literal_and_struct():
    import polars_strsim as ps
    a = ["jonh", "abcd", None, "müller", "", "kitten"]
    b = ["mr john smith", "XXabcdXX", "x", "herr mülelr, k.", "", "sitting"]
    df = pl.DataFrame({"a": a, "b": b}, schema={"a": pl.Utf8, "b": pl.Utf8})
    out = df.select(ps.partial_ratio(pl.col("a"), pl.col("b"))).to_series()
    assert out.name == "a" and out.dtype == pl.Float64
    al = df.select(ps.partial_ratio_alignment(pl.col("a"), pl.col("b"))).to_series()
    assert al.name == "a" and al.dtype == pl.Struct({"score": pl.Float64, "src_start": pl.UInt32, "src_end": pl.UInt32,
                                                     "dest_start": pl.UInt32, "dest_end": pl.UInt32})
    for i, (got, st) in enumerate(zip(out.to_list(), al.to_list())):
        if a[i] is None:
            assert got is None and (st is None or st["score"] is None)
        else:
            want = R.partial(a[i], b[i])
            assert np.float64(got).view(np.uint64) == np.float64(want[0]).view(np.uint64)
            assert (st["score"], st["src_start"], st["src_end"], st["dest_start"], st["dest_end"]) == want
    lit = df.select(ps.partial_ratio(pl.col("b"), pl.lit("jonh"))).to_series().to_list()
    assert lit[0] == 0.75
