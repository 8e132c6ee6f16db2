"""Host side of the Manhattan-frame evaluation (ncnerf_amd.evaluation), no GPU: the faiss draws of
ncn_kmeans_draws against the oracle's faiss_training_set, the selection / relabel table against the
reference's _normals_clustering (tests/golden/normals_clustering_eval.npz, make_golden_eval.py),
the SO(3) projection, and the refusals."""
import os

import numpy as np
import pytest
import torch

from oracle import losses_ref
from ncnerf_amd import evaluation as E
from ncnerf_amd._lib import NcnError

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("K,nx", [(30, 30), (30, 31), (30, 7680), (30, 7681), (30, 12548), (10, 2560), (10, 2561)])
def test_kmeans_draws_match_oracle(K, nx):
    sub, init, rows = E.kmeans_draws(nx, K, seed=1234)
    sub_ref, init_ref = losses_ref.faiss_training_set(nx, K, seed=1234)
    assert sub.dtype == np.int64 and init.dtype == np.int64 and rows.dtype == np.int64
    assert np.array_equal(sub, sub_ref)
    assert np.array_equal(init, init_ref)
    # what spherical_kmeans hands the training kernel: the picks as rows of the training set
    assert rows.min() >= 0 and rows.max() < len(sub) and np.array_equal(sub[rows], init_ref)


def test_kmeans_draws_large_count_is_sparse():
    """Only the first 256 K swap steps are walked: 50 M points cost no 50 M-entry permutation, and
    the entries are distinct indices below nx."""
    nx = 50_000_000
    sub, init, rows = E.kmeans_draws(nx, 30)
    assert len(np.unique(sub)) == 7680 and sub.min() >= 0 and sub.max() < nx
    assert np.isin(init, sub).all() and len(np.unique(init)) == 30
    assert np.array_equal(sub[rows], init)


def test_kmeans_rand_floats_match_oracle():
    assert np.array_equal(E.kmeans_rand_floats(1234, 4096), losses_ref.rand_floats(1234, 4096))


def test_selection_reproduces_reference():
    g = np.load(os.path.join(GOLD, "normals_clustering_eval.npz"))
    C, assign = g["centroids"], g["assign"].astype(np.int64)
    counts = np.bincount(assign, minlength=C.shape[0])
    sim = C @ C.T  # the fixture's premise: two merge pairs, one opposite pair
    iu = np.triu_indices(C.shape[0], 1)
    assert int((sim[iu] > 0.99).sum()) == 2 and int((sim[iu] < -0.99).sum()) == 1
    seen = set()
    for tag, merge, opp in (("TF", True, False), ("TT", True, True), ("FF", False, False)):
        table, picks = E.select_clusters(C, counts, float(g["t_similar"]), merge, opp)
        labels = table[assign]
        assert np.array_equal(labels, g["labels_" + tag].astype(np.int64)), tag
        assert np.array_equal(C[list(picks)], g["centrs_" + tag]), tag
        seen.add(labels.tobytes())
    assert len(seen) == 3  # the flags matter on this input
    # the oracle's selection (merge and opposites on) is the same function
    lab, cn = losses_ref.cluster_select(C, assign, 0.99)
    assert np.array_equal(lab, g["labels_TT"]) and np.array_equal(cn, g["centrs_TT"])


def _rotation(seed):
    from scipy.spatial.transform import Rotation
    return Rotation.random(random_state=seed).as_matrix()


def test_manhattan_frame_recovers_permuted_flipped_rotation():
    R = _rotation(5)
    cents = np.stack([-R[:, 2], R[:, 0], -R[:, 1]]).astype(np.float32)  # centroids = rows, any order / sign
    F, ang = E.manhattan_frame(torch.from_numpy(cents), R_ref=torch.from_numpy(R))
    assert np.abs(F - R).max() <= 1e-6
    assert np.abs(np.linalg.det(F) - 1.0) <= 1e-6 and np.abs(F.T @ F - np.eye(3)).max() <= 1e-6
    assert ang.shape == (3,) and ang.max() < 0.05  # (f32 centroids: arccos near 1)
    # without a reference the centroids are projected in order
    F2, ang2 = E.manhattan_frame(np.stack([R[:, 0], R[:, 1], R[:, 2]]))
    assert ang2 is None and np.abs(F2 - R).max() <= 1e-6


def test_manhattan_frame_projects_noisy_centroids():
    R = _rotation(9)
    rng = np.random.default_rng(0)
    cents = R.T + rng.normal(0, 0.02, (3, 3))
    F, ang = E.manhattan_frame(cents, R_ref=R)
    assert np.abs(F.T @ F - np.eye(3)).max() <= 1e-9 and np.linalg.det(F) > 0
    assert ang.max() < 3.0


def test_too_few_normals_raise():
    with pytest.raises(ValueError):
        E.kmeans_draws(29, 30)
    L = E._lib.lib()
    sub, init = np.zeros(64, np.int64), np.zeros(64, np.int64)
    assert L.ncn_kmeans_draws(29, 30, 1234, sub.ctypes.data, init.ctypes.data, None) != 0
    assert b"29 points" in L.ncn_last_error()
    assert L.ncn_kmeans_draws(31, 30, 1234, sub.ctypes.data, init.ctypes.data, None) == 0  # init_rows is optional
    with pytest.raises(RuntimeError):  # a host tensor is refused before anything else (the N < K
        E.normals_clustering(torch.zeros(29, 3), K=30)  # refusal on the device: test_gpu_eval.py)
    with pytest.raises(NcnError):
        E.kmeans_draws(100, 33)  # K beyond the kernels' 32


def test_module_is_exported():
    import ncnerf_amd
    assert "evaluation" in ncnerf_amd.__all__
