"""polars_strsim.indel / indel_distance through a REAL Polars engine.  Polars is not in every image: without it this file skips."""
import inspect

import numpy as np
import pytest

pl = pytest.importorskip("polars")

import indel_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_wrapper_signatures_and_all():
    import polars_strsim as ps
    assert "indel" in ps.__all__ and "indel_distance" in ps.__all__
    assert list(inspect.signature(ps.indel).parameters) == ["expr", "other"]
    assert list(inspect.signature(ps.indel_distance).parameters) == ["expr", "other", "max_distance"]
    assert inspect.signature(ps.indel_distance).parameters["max_distance"].default is None
    for doc in (ps.indel.__doc__, ps.indel_distance.__doc__):
        assert "fuzz.ratio" in doc and "substitution costs 2" in doc and "upstream polars-strsim" in doc
    for args in (("a", "b"), (pl.col("a"), pl.lit("x")), (pl.lit("x"), "b")):
        assert isinstance(ps.indel(*args), pl.Expr) and isinstance(ps.indel_distance(*args, max_distance=2), pl.Expr)
    with pytest.raises(ValueError):
        ps.best_match("indel", "a", "b")
    with pytest.raises(ValueError):
        ps.nearest("indel", "a", "b")


def test_indel_column_literal_and_cutoff():
    import polars_strsim as ps
    a = ["jonh", "martha", None, "müller", "", "kitten"]
    b = ["john", "marhta", "x", "mülelr", "", "sitting"]
    df = pl.DataFrame({"a": a, "b": b}, schema={"a": pl.Utf8, "b": pl.Utf8})
    out = df.select(ps.indel(pl.col("a"), pl.col("b"))).to_series()
    assert out.name == "a" and out.dtype == pl.Float64
    for i, got in enumerate(out.to_list()):
        if a[i] is None:
            assert got is None
        else:
            assert np.float64(got).view(np.uint64) == np.float64(R.score(a[i], b[i])).view(np.uint64)
    d = df.select(ps.indel_distance(pl.col("a"), pl.col("b"))).to_series()
    assert d.name == "a" and d.dtype == pl.UInt32 and d.to_list() == [2, 2, None, 2, 0, 5]
    assert df.select(ps.indel_distance(pl.col("a"), pl.col("b"), max_distance=2)).to_series().to_list() == [2, 2, None, 2, 0, 3]
    lit = df.select(ps.indel(pl.col("b"), pl.lit("jonh"))).to_series().to_list()
    assert lit[0] == 0.75
