"""The two host paths to faiss's k-means draws make the same draws: the training step's plan
(ncn_kmeans_plan_fill, one row per point count) and the evaluation's ncn_kmeans_draws (one point
count per call) read one Fisher-Yates prefix and one rand_float statement (csrc/kmeans_faiss.h).
Host code only, no GPU call."""
import numpy as np
import pytest
import torch

from ncnerf_amd import _lib
from ncnerf_amd import evaluation as E

N_RAND = 4096
_PLANS = {}


def _plan(n_tri, K):
    if (n_tri, K) not in _PLANS:  # built once per case set
        buf = torch.zeros(int(_lib.lib().ncn_kmeans_plan_words(n_tri, K)), dtype=torch.int32)
        assert _lib.call("ncn_kmeans_plan_fill", n_tri, K, 1234, buf) == 0
        _PLANS[(n_tri, K)] = buf.numpy().view(np.uint32)
    return _PLANS[(n_tri, K)]


def _cases():
    for n_tri, K in ((6272, 20), (3000, 10)):
        cap = K * 256
        for nx in (K, K + 1, 57, cap, cap + 1, n_tri):
            yield pytest.param(n_tri, K, nx, id=f"n{n_tri}-K{K}-nx{nx}")


@pytest.mark.parametrize("n_tri,K,nx", list(_cases()))
def test_plan_and_eval_draws_agree(n_tri, K, nx):
    p = _plan(n_tri, K)
    cap, mw = K * 256, (n_tri + 31) // 32
    sub, init, _rows = E.kmeans_draws(nx, K, seed=1234)
    picks = p[p[5]:p[6]].view(np.uint16)[nx * K:(nx + 1) * K].astype(np.int64)
    if nx == K:
        # faiss's nx == k corner case: both kernels copy the points in order and read no init pick
        # (the plan states that order; ncn_kmeans_draws' picks are a permutation of the same points)
        assert np.array_equal(picks, np.arange(K)) and np.array_equal(sub, np.arange(K))
        assert np.array_equal(np.sort(init), picks)
    else:
        assert np.array_equal(picks, init)
    if nx > cap:
        row = p[p[6] + (nx - cap - 1) * mw:p[6] + (nx - cap) * mw]
        members = np.flatnonzero(np.unpackbits(row.view(np.uint8), bitorder="little"))
        assert len(sub) == cap and np.array_equal(members, np.sort(sub))
    else:
        assert np.array_equal(sub, np.arange(nx))
    rnd = p[p[7]:p[7] + N_RAND].view(np.float32)
    assert p[4] == N_RAND and np.array_equal(rnd, E.kmeans_rand_floats(1234, N_RAND))
