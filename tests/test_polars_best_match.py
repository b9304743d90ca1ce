"""polars_strsim.best_match through a REAL Polars engine.  Polars is not in every image: without it this file skips, and the first
box that has it runs it (python -m pytest tests/test_polars_best_match.py -m gpu -q)."""
import numpy as np
import pytest

pl = pytest.importorskip("polars")

import best_match_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("measure", ["levenshtein", "jaro_winkler"])
def test_best_match_column_against_a_shorter_candidate_column(measure):
    import polars_strsim as ps
    names = ["apple", "banana", None, "cherry", "kiwi"]
    cands = ["banan", None, "appel", "chery", "kiwi", "apple"]
    df = pl.DataFrame({"name": names}, schema={"name": pl.Utf8})
    out = df.select(ps.best_match(pl.col("name"), pl.lit(pl.Series(cands, dtype=pl.Utf8)), measure=measure)).to_series()
    assert out.name == "name"
    pos = [j for j, c in enumerate(cands) if c is not None]
    idx, val = R.topk(R.score_matrix(measure, [n or "" for n in names], [cands[j] for j in pos]), 1)
    for i, got in enumerate(out.to_list()):
        if names[i] is None:
            assert got is None
        else:
            assert got["index"] == pos[idx[i, 0]]
            assert np.float64(got["score"]).view(np.uint64) == np.float64(val[i, 0]).view(np.uint64)
