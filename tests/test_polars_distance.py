"""polars_strsim.levenshtein_distance / osa_distance through a REAL Polars engine.  Polars is not in every image: without it this
file skips."""
import pytest

pl = pytest.importorskip("polars")

import distance_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_distance_wrappers_column_literal_and_cutoff():
    import polars_strsim as ps
    a = ["kitten", "abcd", None, "ca", "héllo"]
    b = ["sitting", "acbd", "x", "abc", ""]
    df = pl.DataFrame({"a": a, "b": b}, schema={"a": pl.Utf8, "b": pl.Utf8})
    lev = df.select(ps.levenshtein_distance(pl.col("a"), pl.col("b"))).to_series()
    assert lev.name == "a" and lev.dtype == pl.UInt32
    assert lev.to_list() == [3, 2, None, 3, 5]
    assert df.select(ps.osa_distance(pl.col("a"), pl.col("b"))).to_series().to_list() == [3, 1, None, 3, 5]
    assert df.select(ps.osa_distance(pl.col("a"), pl.col("b"), max_distance=1)).to_series().to_list() == [2, 1, None, 2, 2]
    lit = df.select(ps.levenshtein_distance(pl.col("b"), pl.lit("abc"), max_distance=2)).to_series().to_list()
    assert lit == [R.distance("levenshtein", s, "abc", 2) for s in b]
    assert "levenshtein_distance" in ps.__all__ and "osa_distance" in ps.__all__
