"""polars_strsim.nearest through a REAL Polars engine.  Polars is not in every image: without it this file skips."""
import pytest

pl = pytest.importorskip("polars")

pytestmark = pytest.mark.gpu


def test_polars_nearest_struct_nulls_and_cutoff():
    import polars_strsim as ps
    df = pl.DataFrame({"q": ["kitten", None, "abc", "zzzz"]}, schema={"q": pl.Utf8})
    cands = pl.Series("c", [None, "sitting", "abd", None, "kitten"], dtype=pl.Utf8)
    out = df.select(ps.nearest(pl.col("q"), cands)).to_series()
    assert out.name == "q"
    assert out.to_list() == [{"index": 4, "distance": 0}, None, {"index": 2, "distance": 1}, {"index": 2, "distance": 4}]
    out = df.select(ps.nearest(pl.col("q"), cands, measure="osa", max_distance=1)).to_series()
    assert out.to_list() == [{"index": 4, "distance": 0}, None, {"index": 2, "distance": 1}, None]
    with pytest.raises(ValueError):
        ps.nearest(pl.col("q"), cands, measure="jaro")
    assert "nearest" in ps.__all__
