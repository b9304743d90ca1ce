"""polars_strsim.default_process through a REAL Polars engine (skipped without Polars, like tests/test_polars_wrappers.py):

    pip install 'polars>=1,<2' && python -m pytest tests/test_polars_process.py -m gpu -q
"""
import inspect

import numpy as np
import pytest

pl = pytest.importorskip("polars")

import process_ref as R  # noqa: E402


def test_wrapper_signature_and_all():
    import polars_strsim as ps
    assert ps.__all__[0] == "default_process"
    assert list(inspect.signature(ps.default_process).parameters) == ["expr"]
    assert "utils.default_process" in ps.default_process.__doc__ and "upstream polars-strsim" in ps.default_process.__doc__
    for arg in ("name", pl.col("name"), pl.lit("Apple, Inc.")):
        assert isinstance(ps.default_process(arg), pl.Expr)


@pytest.mark.gpu
def test_default_process_column_and_composition():
    import polars_strsim as ps
    a = ["Apple, Inc.", None, "ÀÉ　x", "!!!", "", "ȺȾ" * 40]
    b = ["apple inc", "x", None, "", "?", "ⱥⱦ" * 40]
    df = pl.DataFrame({"a": a, "b": b}, schema={"a": pl.Utf8, "b": pl.Utf8})
    out = df.select(ps.default_process(pl.col("a")))
    assert out.schema == {"a": pl.String} and out.to_series().to_list() == [R.default_process(s) for s in a]
    lazy = df.lazy().select(ps.default_process("b")).collect().to_series().to_list()
    assert lazy == [R.default_process(s) for s in b]
    score = df.select(ps.indel(ps.default_process("a"), ps.default_process("b"))).to_series().to_list()
    assert score[0] == 1 - 1 / 19 and score[1] is None and score[2] is None and score[5] == 1.0
    raw = df.select(ps.indel("a", "b")).to_series().to_list()
    assert np.float64(raw[0]) == 0.7
    assert df.head(0).select(ps.default_process("a")).to_series().to_list() == []
