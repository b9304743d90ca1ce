"""polars_strsim.osa through a REAL Polars engine.  Polars is not in every image: without it this file skips."""
import numpy as np
import pytest

pl = pytest.importorskip("polars")

import osa_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_osa_column_and_literal():
    import polars_strsim as ps
    a = ["jonh", "martha", None, "müller", ""]
    b = ["john", "marhta", "x", "mülelr", ""]
    df = pl.DataFrame({"a": a, "b": b}, schema={"a": pl.Utf8, "b": pl.Utf8})
    out = df.select(ps.osa(pl.col("a"), pl.col("b"))).to_series()
    assert out.name == "a"
    for i, got in enumerate(out.to_list()):
        if a[i] is None:
            assert got is None
        else:
            assert np.float64(got).view(np.uint64) == np.float64(R.score(a[i], b[i])).view(np.uint64)
    lit = df.select(ps.osa(pl.col("b"), pl.lit("jonh"))).to_series().to_list()
    assert lit[0] == 0.75
