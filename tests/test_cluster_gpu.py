"""strsim_cluster_device / _host and strsim_amd.cluster on the GPU, exact against tests/cluster_ref.py (the union-find over the hits
of join_ref / match_join_ref): root, cluster and count of every row, and the number of pairs of the self-join.  Every frame is first
shown ON THE MODEL to be worth clustering: clusters of several members, one of which holds a pair that is not itself a hit, and edges
that only the join's slow fallback can have found."""
import functools

import numpy as np
import pytest

import cluster_frames as F
import cluster_ref as R
import gen
import strsim_amd as S

pytestmark = pytest.mark.gpu
INF = float("inf")
SEED = 41


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def model(measure):
    """(column, min_score, hits, (root, cluster, count, nnz)) of the measure's frame: computed once, shared, never changed"""
    col = tuple(F.frame(SEED))
    cut = F.MIN_SCORE[measure]
    found = R.hits(measure, col, cut)
    return col, cut, found, R.cluster(measure, col, cut, found)


def _device_column(torch, col):
    off, val = S.pack_strings(list(col))
    dev = torch.device("cuda", 0)
    out = torch.from_numpy(off.view(np.int32)).to(dev), torch.from_numpy(val).to(dev)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("measure", R.CLUSTER_MEASURES)
def test_cluster_gpu_frame_against_the_model(ctx, measure):
    torch = pytest.importorskip("torch")
    col, cut, found, exp = model(measure)
    # the frame is worth it, on the model alone
    assert R.worth_it(measure, col, cut, found)
    indptr, index, _ = found
    slow = [gen.outside_lane_class(s, measure == "token_sort_ratio") for s in col]
    assert any(slow[u] or slow[int(index[e])] for u in range(len(col)) for e in range(int(indptr[u]), int(indptr[u + 1])))
    assert 3 < exp[2] < len(col) - 3
    # host entry point
    off, val = S.pack_strings(list(col))
    root, cluster, count, nnz = ctx.cluster(R.MEASURE[measure], off, val, cut, with_nnz=True)
    assert root.dtype == cluster.dtype == np.uint32
    assert nnz == exp[3] and count == exp[2]
    assert root.tolist() == exp[0] and cluster.tolist() == exp[1]
    # device entry point
    root, cluster, count, nnz = ctx.cluster(R.MEASURE[measure], *_device_column(torch, col), cut, with_nnz=True)
    assert root.is_cuda and cluster.is_cuda
    assert nnz == exp[3] and count == exp[2]
    assert root.cpu().tolist() == exp[0] and cluster.cpu().tolist() == exp[1]
    # the Python surface: int64, the same labels
    root, cluster, count = S.cluster(measure, list(col), cut, ctx=ctx)
    assert root.dtype == cluster.dtype == np.int64 and count == exp[2]
    assert root.tolist() == exp[0] and cluster.tolist() == exp[1]


@pytest.mark.parametrize("measure", ["jaro_winkler", "ratio"])
def test_cluster_gpu_more_pairs_than_the_first_capacity(ctx, measure):
    # 200 copies of each of 5 strings: 5 * C(200, 2) = 99 500 pairs > 4 * 1000 + 1024, so the join is made a second time
    base = ["margaret thatcher", "winston churchill", "clement attlee", "harold wilson", "edward heath"]
    col = [base[i % 5] for i in range(1000)]
    assert 5 * 200 * 199 // 2 > 4 * len(col) + 1024
    off, val = S.pack_strings(col)
    root, cluster, count, nnz = ctx.cluster(R.MEASURE[measure], off, val, 0.95, with_nnz=True)
    assert nnz == 5 * 200 * 199 // 2 and count == 5
    assert root.tolist() == [i % 5 for i in range(1000)] and cluster.tolist() == [i % 5 for i in range(1000)]
    # once more on the same context (the buffer has grown: one join now would do, the answer is the same)
    assert ctx.cluster(R.MEASURE[measure], off, val, 0.95, with_nnz=True)[2:] == (5, nnz)


@pytest.mark.parametrize("measure", R.CLUSTER_MEASURES)
def test_cluster_gpu_min_score_above_one_and_minus_infinity(ctx, measure):
    col = list(model(measure)[0])[:70]
    off, val = S.pack_strings(col)
    n = len(col)
    root, cluster, count, nnz = ctx.cluster(R.MEASURE[measure], off, val, 1.5, with_nnz=True)
    assert nnz == 0 and count == n and root.tolist() == list(range(n)) and cluster.tolist() == list(range(n))
    root, cluster, count, nnz = ctx.cluster(R.MEASURE[measure], off, val, -INF, with_nnz=True)
    assert nnz == n * (n - 1) // 2 and count == 1 and not root.any() and not cluster.any()
    with pytest.raises(S.StrsimError, match="min_score is NaN"):
        ctx.cluster(R.MEASURE[measure], off, val, float("nan"))


def test_cluster_gpu_single_row_and_empty_column(ctx):
    off, val = S.pack_strings(["solo"])
    assert [x if isinstance(x, int) else x.tolist() for x in ctx.cluster("jaro", off, val, 0.5, with_nnz=True)] == [[0], [0], 1, 0]
    off, val = S.pack_strings([])
    root, cluster, count = ctx.cluster("indel", off, val, 0.5)
    assert root.size == 0 and cluster.size == 0 and count == 0


def test_cluster_gpu_nulls_never_join_anything(ctx):
    col = ["anna", None, "", "ana", None, "bob", "", "anna", None, "bobb"]
    root, cluster, count = S.cluster("ratio", col, 0.8, ctx=ctx)
    assert root.tolist() == [0, -1, 2, 0, -1, 5, 2, 0, -1, 5]
    assert cluster.tolist() == [0, -1, 1, 0, -1, 2, 1, 0, -1, 2] and count == 3
    root, cluster, count = S.cluster("levenshtein", [None, None], 0.8, ctx=ctx)
    assert root.tolist() == [-1, -1] and count == 0
    # against the model over the non-null rows of a frame
    full = list(model("jaro_winkler")[0])
    col = [None if i % 6 == 2 else s for i, s in enumerate(full)]
    pos = [i for i, s in enumerate(col) if s is not None]
    exp = R.cluster("jaro_winkler", [col[i] for i in pos], 0.92)
    root, cluster, count = S.cluster("jaro_winkler", col, 0.92, ctx=ctx)
    assert count == exp[2]
    assert [root[i] for i in pos] == [pos[r] for r in exp[0]] and [cluster[i] for i in pos] == exp[1]
    assert all(root[i] == -1 and cluster[i] == -1 for i in range(len(col)) if col[i] is None)


def test_cluster_gpu_default_process_merges_spellings(ctx):
    col = ["Apple, Inc.", "banana", "apple inc", "  BANANA!", "cherry"]
    root, cluster, count = S.cluster("ratio", col, 0.9, ctx=ctx)
    assert root.tolist() == [0, 1, 2, 3, 4] and count == 5
    root, cluster, count = S.cluster("ratio", col, 0.9, ctx=ctx, processor="default_process")
    assert root.tolist() == [0, 1, 0, 1, 4] and cluster.tolist() == [0, 1, 0, 1, 2] and count == 3
