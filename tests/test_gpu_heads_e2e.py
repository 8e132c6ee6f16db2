"""The semantic / normal heads end to end on a small synthetic scene (256 rays, 5 classes): render()'s
train and test paths, the semantic term of NeRFMTLoss, and the Trainer in eager and graph mode.

Tolerances: rgb / depth / opacity of a heads-on model equal the heads-off model's bit for bit (the
heads read the field, they do not touch it).  Graph against eager: tests/test_gpu_graph.py's bounds
for graph == eager (per-step loss within 1e-4 relative; hash-table entries moved by more than 1e-4
at most 5e-5 of them and by more than 1e-6 under 0.1 %, the float-atomic floor of the table-gradient
flush; every MLP weight, the heads' included, within 1e-3 relative L2)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ncnerf_amd.losses import NeRFMTLoss
from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
from ncnerf_amd.rendering import render
from ncnerf_amd.synthetic import SyntheticScene
from ncnerf_amd.trainer import HYPERSIM_HPARAMS, Trainer

pytestmark = pytest.mark.gpu
R, K = 256, 5
HPARAMS = dict(loss_sem_w=0.1, pred_sem=True, load_sem_gt=True)


@pytest.fixture(scope="module")
def scene():
    return SyntheticScene()


def _model(dev, scene, heads=True, seed=7):
    torch.manual_seed(seed)
    kw = dict(pred_sem=True, n_sem_cls=K, pred_norm=True) if heads else {}
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128, **kw).to(dev))
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-1e-2, 1e-2)
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    return m


def _batch(scene, dev, seed):
    b = scene.torch_batch(R, seed=seed, device=dev)
    b["march_noise"] = torch.rand(R, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    # labels 1..K from the target colour (learnable from the ray), 0 = void on every seventh ray
    lab = 1 + torch.clamp((b["rgb"][:, 0] * K).long(), 0, K - 1)
    lab[::7] = 0
    b["semantics"] = lab
    return b


@pytest.mark.parametrize("test_time", [False, True])
def test_render_with_heads(dev, scene, test_time):
    m, m0 = _model(dev, scene), _model(dev, scene, heads=False)
    with torch.no_grad():
        m0.flat_params().copy_(m.flat_params()[:m0.flat_params().numel()])
    b = _batch(scene, dev, 3)
    kw = dict(near_distance=0.01, max_samples=1024, test_time=test_time)
    if not test_time:
        kw["march_noise"] = b["march_noise"]
    with torch.no_grad():
        r = render(m, b["rays_o"], b["rays_d"], n_sem_cls=K, **kw)
        r0 = render(m0, b["rays_o"], b["rays_d"], **kw)
        rn = render(m, b["rays_o"], b["rays_d"], n_sem_cls=K, pred_norm_nn_norm=True, **kw)
    assert r["sem"].shape == (R, K) and r["norm_nn"].shape == (R, 3)
    assert torch.isfinite(r["sem"]).all() and torch.isfinite(r["norm_nn"]).all()
    assert float(r["sem"].abs().max()) > 0 and float(r["norm_nn"].abs().max()) > 0
    for k in ("rgb", "depth", "opacity"):
        assert torch.equal(r[k], r0[k]), k
    hit = r["norm_nn"].norm(dim=1) > 1e-6
    np.testing.assert_allclose(rn["norm_nn"][hit].norm(dim=1).cpu().numpy(), 1.0, rtol=1e-5)


def test_static_render_with_heads_matches_dynamic(dev, scene):
    m = _model(dev, scene)
    b = _batch(scene, dev, 4)
    kw = dict(near_distance=0.01, max_samples=1024, march_noise=b["march_noise"], n_sem_cls=K)
    with torch.no_grad():
        r0 = render(m, b["rays_o"], b["rays_d"], **kw)
        r1 = render(m, b["rays_o"], b["rays_d"], static_shapes=True, **kw)
    for k in ("rgb", "depth", "opacity", "sem", "norm_nn"):  # (the capacity tail reaches no result)
        assert torch.equal(r0[k], r1[k]), k


def test_semantic_loss_term(dev, scene):
    m = _model(dev, scene)
    b = _batch(scene, dev, 5)
    loss = NeRFMTLoss(dict(HYPERSIM_HPARAMS, **HPARAMS))
    res = render(m, b["rays_o"], b["rays_d"], near_distance=0.01, max_samples=1024, march_noise=b["march_noise"],
                 n_sem_cls=K)
    ld = loss(res, b, global_step=1000)
    want = 0.1 * F.cross_entropy(res["sem"].detach().float(), b["semantics"] - 1, ignore_index=-1)
    np.testing.assert_allclose(float(ld["sem"].detach()), float(want), rtol=1e-5)
    assert float(ld["sem"].detach()) > 0
    np.testing.assert_allclose(float(ld["total"].detach()),
                               sum(float(v.detach()) for k, v in ld.items() if k != "total"), rtol=1e-5)
    # an all-void batch: exactly 0, exactly zero and finite gradients
    void = dict(b, semantics=torch.zeros_like(b["semantics"]))
    ld = loss(res, void, global_step=1000)
    (g,) = torch.autograd.grad(ld["sem"], res["sem"], retain_graph=True)
    assert float(ld["sem"].detach()) == 0.0 and torch.isfinite(g).all() and float(g.abs().max()) == 0.0
    m.flat_grad().zero_()
    ld["sem"].backward()
    torch.cuda.synchronize()
    fg = m.flat_grad()
    assert torch.isfinite(fg).all() and float(fg.abs().max()) == 0.0


def test_trainer_graph_matches_eager_with_heads(dev, scene):
    """Ten Trainer steps with use_graph=True against ten eager steps on the same batches and jitter; two
    eager runs give the run-to-run floor."""
    batches = [_batch(scene, dev, 50 + k) for k in range(10)]
    losses, sems, params = [], [], []
    for use_graph in (False, False, True):
        m = _model(dev, scene)
        tr = Trainer(m, hparams=HPARAMS, update_grid=False, use_graph=use_graph)
        assert tr.render_kwargs["n_sem_cls"] == K and not tr.opt.pack_fused
        ls, ss = [], []
        for k, b in enumerate(batches):
            _, ld = tr.step(b, global_step=1000 + 200 * k)  # inside the clustering ramp
            ls.append(float(ld["total"].detach()))
            ss.append(float(ld["sem"].detach()))
        torch.cuda.synchronize()
        assert tr._split is None  # (a model with heads takes the autograd body)
        losses.append(np.array(ls))
        sems.append(np.array(ss))
        params.append(m.flat_params().detach().clone())
    assert np.isfinite(losses[0]).all() and (sems[0] > 0).all()
    np.testing.assert_allclose(losses[2], losses[0], rtol=1e-4)
    np.testing.assert_allclose(sems[2], sems[0], rtol=1e-4)
    n_t = m._n_table
    for other in (1, 2):
        d = (params[other][:n_t] - params[0][:n_t]).abs()
        assert int((d > 1e-4).sum()) <= 5e-5 * n_t, other
        assert float((d > 1e-6).float().mean()) < 1e-3, other
    rel_w = float((params[2][n_t:] - params[0][n_t:]).norm() / params[0][n_t:].norm())
    assert rel_w < 1e-3, rel_w
    assert not torch.equal(params[0][n_t + 10240:], _model(dev, scene).flat_params()[n_t + 10240:])  # the heads moved


def test_semantic_loss_decreases(dev, scene):
    """The `sem` loss after 50 steps on a fixed batch is below its value at step 0."""
    m = _model(dev, scene)
    tr = Trainer(m, hparams=HPARAMS, update_grid=False, use_graph=True)
    b = _batch(scene, dev, 9)
    sem = []
    for k in range(51):
        res, ld = tr.step(b, global_step=1000 + k)
        sem.append(float(ld["sem"].detach()))
        assert torch.isfinite(res["sem"]).all(), k  # (the validity filter would turn a NaN term into a 0)
    print(f"sem loss: step 0 {sem[0]:.5f}, step 50 {sem[50]:.5f}")
    assert np.isfinite(sem).all() and sem[50] < sem[0]
