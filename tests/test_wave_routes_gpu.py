"""The routes inside k_wave_pairs<M>, on one small frame (tests/wave_frames.py; tests/test_wave_frames_cpu.py checks what it holds).

Every row of the frame is left to the wave kernel.  Its Levenshtein body deals the rows into ASCII batches, 16-bit-symbol batches,
the fallback for scalar values beyond the BMP, the early return of an empty side and the rows left to k_huge_pairs; the body of
the other four measures runs them one by one.  Every measure, as column x column and with a one-row side on either side, must
agree with the oracle bit for bit in every row.
"""
import numpy as np
import pytest

import wave_frames as W
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import strsim_amd
    return strsim_amd


@pytest.fixture(scope="module")
def ctx(S):
    c = S.Context(0)
    yield c
    c.close()


def run(S, ctx, measure, literal_side=None, literal=None):
    A, B = W.sides(literal_side, literal)
    ao, av = S.pack_strings(list(A))
    bo, bv = S.pack_strings(list(B))
    got = ctx.pairs_host(measure, ao, av, bo, bv)
    exp = W.expected(measure, literal_side, literal)
    assert len(got) == len(exp) == len(W.frame().A)
    bad = np.nonzero(np.asarray(got, dtype=np.float64).view(np.uint64) != exp.view(np.uint64))[0]
    if bad.size:
        f = W.frame()
        i = int(bad[0])
        cls = [name for name, r in f.classes.items() if i in r][0]
        raise AssertionError(f"{measure} literal {literal_side}/{literal}: {bad.size}/{len(exp)} rows differ; first row {i} ({cls}): "
                             f"a={A[i if len(A) > 1 else 0][:40]!r}.. b={B[i if len(B) > 1 else 0][:40]!r}.. got={got[i]!r} exp={exp[i]!r}")


@pytest.mark.parametrize("measure", O.MEASURES)
def test_column_against_column(S, ctx, measure):
    run(S, ctx, measure)
    assert ctx.last_wave_rows == len(W.frame().A)  # every row was the wave kernel's, the rows it left to k_huge_pairs included


@pytest.mark.parametrize("literal", sorted(W.LITERALS))
@pytest.mark.parametrize("literal_side", ["a", "b"])
@pytest.mark.parametrize("measure", O.MEASURES)
def test_column_against_literal(S, ctx, measure, literal_side, literal):
    run(S, ctx, measure, literal_side, literal)
