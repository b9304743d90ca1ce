"""qgram_cluster on the MI355X (strsim_qgram_cluster_*): the labels must equal tests/cluster_ref.py's union-find over the reference
CSR of tests/qgram_join_ref.py, exactly.  The frame holds a chain a ~ b ~ c whose ends do not match each other."""
import numpy as np
import pytest

import cluster_ref
import qgram_join_frames as F
import qgram_join_ref as R

pytestmark = pytest.mark.gpu

S = pytest.importorskip("strsim_amd")


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def _model(kind, q, multiset, cut):
    X = list(F.cluster_column())
    found = R.join(kind, X, X, cut, q, multiset, True)
    return X, found, cluster_ref.cluster(None, X, cut, found=found)


def test_qgram_cluster_gpu_chain_whose_ends_do_not_match(ctx):
    X, (ep, ei, es), (root, label, count, nnz) = _model("sorensen_dice", 2, True, F.CLUSTER_CUT)
    hits = {(i, int(ei[e])): float(es[e]) for i in range(len(X)) for e in range(int(ep[i]), int(ep[i + 1]))}
    assert (0, 1) in hits and (1, 2) in hits and (0, 2) not in hits  # a ~ b ~ c, a and c do not match
    assert cluster_ref.worth_it(None, X, F.CLUSTER_CUT, (ep, ei, es))
    r, c, n, pairs = ctx.qgram_cluster("sorensen_dice", *S.pack_strings(X), F.CLUSTER_CUT, with_nnz=True)
    assert r.dtype == np.uint32 and r.tolist() == root and c.tolist() == label and n == count and pairs == nnz
    assert r[0] == r[1] == r[2] == 0


@pytest.mark.parametrize("kind,q,multiset,cut", [("jaccard", 2, True, 0.7), ("jaccard", 3, False, 0.7), ("overlap", 2, True, 0.9),
                                                 ("cosine", 1, False, 0.95), ("sorensen_dice", 3, True, 0.8)])
def test_qgram_cluster_gpu_labels_equal_the_reference(ctx, kind, q, multiset, cut):
    X, found, (root, label, count, nnz) = _model(kind, q, multiset, cut)
    assert 0 < nnz < len(X) * (len(X) - 1) // 2 and 1 < count < len(X)
    r, c, n, pairs = ctx.qgram_cluster(kind, *S.pack_strings(X), cut, q=q, multiset=multiset, with_nnz=True)
    assert r.tolist() == root and c.tolist() == label and n == count and pairs == nnz


def test_qgram_cluster_gpu_device_columns_nulls_and_the_range_of_min_score(ctx):
    torch = pytest.importorskip("torch")
    X, found, (root, label, count, nnz) = _model("sorensen_dice", 2, True, F.CLUSTER_CUT)
    off, val = S.pack_strings(X)
    dev = torch.device("cuda", 0)
    o, v = torch.from_numpy(off.view(np.int32)).to(dev), torch.from_numpy(val).to(dev)
    r, c, n = ctx.qgram_cluster("sorensen_dice", o, v, F.CLUSTER_CUT)
    ctx.synchronize()
    assert r.is_cuda and r.cpu().numpy().view(np.uint32).tolist() == root and c.cpu().numpy().view(np.uint32).tolist() == label and n == count
    # above 1.0 nothing matches: the identity; 0.0 links everything
    r, c, n = ctx.qgram_cluster("sorensen_dice", off, val, 1.5)
    assert r.tolist() == list(range(len(X))) and n == len(X)
    r, c, n = ctx.qgram_cluster("sorensen_dice", off, val, 0.0)
    assert not r.any() and n == 1
    # the Python surface: a null row never joins anything
    col = ["night", None, "nights", "nacht", None, "night"]
    root, label, count = S.qgram_cluster("sorensen_dice", col, 0.8, ctx=ctx)
    assert root.tolist() == [0, -1, 0, 3, -1, 0] and label.tolist() == [0, -1, 0, 1, -1, 0] and count == 2
