"""distance_cluster on the MI355X (strsim_distance_cluster_*): the labels must equal tests/cluster_ref.py's union-find over the
reference CSR of tests/distance_join_ref.py, exactly.  The frame holds a chain a ~ b ~ c whose ends are more than k edits apart."""
import numpy as np
import pytest

import cluster_ref
import distance_join_frames as F
import distance_join_ref as R

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def _model(measure, k):
    X = list(F.cluster_column())
    D = R.matrix(measure, X, X)
    found = R.from_distances(D, k, True)
    return X, D, found, cluster_ref.cluster(None, X, k, found=found)


@pytest.mark.parametrize("measure", R.MEASURES)
def test_distance_cluster_gpu_chain_whose_ends_are_further_apart(ctx, measure):
    X, D, (ep, ei, ed), (root, label, count, nnz) = _model(measure, F.CLUSTER_K)
    assert D[0, 1] == 2 and D[1, 2] == 2 and D[0, 2] == 4  # a ~ b ~ c, a and c are 4 edits apart
    assert 0 < nnz < len(X) * (len(X) - 1) // 2 and 1 < count < len(X)
    r, c, n, pairs = ctx.distance_cluster(measure, *S.pack_strings(X), F.CLUSTER_K, with_nnz=True)
    assert r.dtype == np.uint32 and r.tolist() == root and c.tolist() == label and n == count and pairs == nnz
    assert r[0] == r[1] == r[2] == 0


@pytest.mark.parametrize("measure,k", [("levenshtein", 1), ("osa", 3), ("damerau_levenshtein", 3), ("damerau_levenshtein", 0)])
def test_distance_cluster_gpu_labels_equal_the_reference(ctx, measure, k):
    X, D, found, (root, label, count, nnz) = _model(measure, k)
    assert 0 < nnz < len(X) * (len(X) - 1) // 2 and 1 < count < len(X)
    r, c, n, pairs = ctx.distance_cluster(measure, *S.pack_strings(X), k, with_nnz=True)
    assert r.tolist() == root and c.tolist() == label and n == count and pairs == nnz


def test_distance_cluster_gpu_device_columns_nulls_and_the_range_of_max_distance(ctx):
    torch = pytest.importorskip("torch")
    X, D, found, (root, label, count, nnz) = _model("damerau_levenshtein", F.CLUSTER_K)
    off, val = S.pack_strings(X)
    dev = torch.device("cuda", 0)
    o, v = torch.from_numpy(off.view(np.int32)).to(dev), torch.from_numpy(val).to(dev)
    r, c, n = ctx.distance_cluster("damerau_levenshtein", o, v, F.CLUSTER_K)
    ctx.synchronize()
    assert r.is_cuda and r.cpu().numpy().view(np.uint32).tolist() == root and c.cpu().numpy().view(np.uint32).tolist() == label and n == count
    # without a cutoff every row is linked to every other: one cluster
    few = S.pack_strings(X[:100])
    for measure in R.MEASURES:
        r, c, n = ctx.distance_cluster(measure, *few, None)
        assert r.shape == (100,) and not r.any() and n == 1
    # the Python surface: a null row never joins anything
    col = ["night", None, "nigth", "nacht", None, "night"]
    root, label, count = S.distance_cluster("osa", col, 1, ctx=ctx)
    assert root.tolist() == [0, -1, 0, 3, -1, 0] and label.tolist() == [0, -1, 0, 1, -1, 0] and count == 2
    root, label, count = S.distance_cluster("levenshtein", ["night", "nigth", "nacht"], 1, ctx=ctx)
    assert root.tolist() == [0, 1, 2] and count == 3  # the swap is two edits there
