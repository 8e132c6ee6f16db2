"""Training and evaluation cluster alike: the same all-valid unit normals through the training step's
clustering kernel (ncn_cluster_loss, out_centroids) and through the evaluation's k-means
(evaluation.spherical_kmeans: ncn_kmeans_draws + ncn_kmeans_train) give bit-identical centroids.
Both read faiss's arithmetic and draws from csrc/kmeans_faiss.h; the cases reach the paths where the
two kernels differ in shape: tiny chunks, the subsample mask against sub_idx, and split_clusters."""
import numpy as np
import pytest
import torch

from ncnerf_amd import _lib
from ncnerf_amd import evaluation as E
from ncnerf_amd import losses as L
from test_gpu_cluster_edges import _launch
from test_gpu_eval import degenerate_normals

pytestmark = pytest.mark.gpu


def _unit_normals(n, seed):
    x = np.random.default_rng(seed).normal(size=(n, 3)).astype(np.float32)
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))


CASES = {
    "tiny-chunks": (lambda: _unit_normals(57, 57), 20, 20),        # several workgroups empty
    "one-past-cap": (lambda: _unit_normals(5121, 5121), 20, 3),    # membership mask and sub_idx
    "split-K20": (lambda: degenerate_normals(600, seed=5), 20, 20),  # empty clusters every round
    "split-K10": (lambda: degenerate_normals(300, seed=5), 10, 20),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cluster_loss_and_eval_kmeans_centroids_bit_identical(dev, case):
    make, K, niter = CASES[case]
    Xd = torch.from_numpy(make()).to(dev)
    _out, _labels, cents, _dn = _launch(dev, Xd, K, niter=niter)
    cents_eval, _assign, _counts = E.spherical_kmeans(Xd, K, niter)
    torch.cuda.synchronize()
    status = L._cluster_workspace(dev, K).view(torch.int32)[int(_lib.lib().ncn_cluster_status_offset(K))]
    assert int(status.item()) == 0
    a, b = cents.cpu().numpy(), cents_eval.cpu().numpy()
    assert not np.isnan(a).any() and not np.isnan(b).any()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
