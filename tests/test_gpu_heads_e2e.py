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
    if test_time:
        _check_heads_against_one_composite(dev, m, b, r, kw)


def _check_heads_against_one_composite(dev, m, b, r, kw):
    """The values of sem / norm_nn at test time: the loop driven once by hand (vren.raymarching_test,
    model(...), the compositor on rgb for the alive decisions) keeps every ray's samples and head outputs;
    one ncn_composite_test_fw call over them, all 3 + 3 + K channels, must give what render() returned.
    No ray of this model comes near opaque (asserted), so both composite the same samples; the loop
    restarts T = 1 - opacity every round where the one call keeps the running product, so the two are
    not the same bits: each is held to the renderer's float bound (tests/render_test_cases.py:
    GPU_C 2^-24 (n_r + 1) max(1, max|v|)) against the float64 sums over those samples."""
    import render_test_cases as rc
    from ncnerf_amd import _lib, vren
    rays_o, rays_d, ms = b["rays_o"].contiguous(), b["rays_d"].contiguous(), kw["max_samples"]
    C = 6 + K
    _, hits_t, _ = vren.ray_aabb_intersect(rays_o, rays_d, m.center, m.half_size, 1, near_distance=kw["near_distance"])
    ht = hits_t[:, 0].contiguous()
    alive = torch.arange(R, device=dev)
    op, de, re = torch.zeros(R, device=dev), torch.zeros(R, device=dev), torch.zeros(R, 3, device=dev)
    samples, rounds = 0, []
    with torch.no_grad(), torch.autocast("cuda"):
        while samples < ms and len(alive):
            NS = max(min(R // len(alive), 64), 1)
            samples += NS
            xyzs, dirs, deltas, ts, n_eff = vren.raymarching_test(rays_o, rays_d, ht, alive, m.density_bitfield,
                                                                  m.cascades, m.scale, 0.0, m.grid_size, ms, NS)
            valid = torch.arange(NS, device=dev)[None, :] < n_eff[:, None]
            if not bool(valid.any()):
                break
            out = m(xyzs[valid], dirs[valid], n_sem_cls=K, **kw)
            sig = torch.zeros(len(alive), NS, device=dev)
            sig[valid] = out["sigmas"].float()
            raws = torch.zeros(len(alive), NS, C, device=dev)
            raws[valid] = torch.cat([out["rgbs"].float(), out["norms"].float(), out["sems"].float()], dim=-1)
            rounds.append((alive.clone(), n_eff, valid, sig, raws, deltas, ts))
            vren.composite_test_multi_fw(sig, raws[..., :3].contiguous(), deltas, ts, ht, alive, 1e-4, n_eff, op, de, re)
            alive = alive[alive >= 0]
    assert torch.equal(op, r["opacity"]) and float(op.max()) < 0.99  # the hand-driven loop is the renderer's
    n = torch.zeros(R, dtype=torch.int64, device=dev)
    for al, n_eff, *_ in rounds:
        n[al] += n_eff
    S = int(n.max())
    big = [torch.zeros(R, S, device=dev), torch.zeros(R, S, C, device=dev), torch.zeros(R, S, device=dev),
           torch.zeros(R, S, device=dev)]
    pos = torch.zeros(R, dtype=torch.int64, device=dev)
    for al, n_eff, valid, *arrays in rounds:
        rows = al[:, None].expand_as(valid)[valid]
        cols = (pos[al][:, None] + torch.arange(valid.shape[1], device=dev)[None, :])[valid]
        for dst, src in zip(big, arrays):
            dst[rows, cols] = src[valid]
        pos[al] += n_eff
    al1 = torch.arange(R, device=dev)
    op1, de1, re1 = torch.zeros(R, device=dev), torch.zeros(R, device=dev), torch.zeros(R, C, device=dev)
    _lib.call("ncn_composite_test_fw", *big, al1, R, S, C, 1e-4, n.int(), op1, de1, re1)
    # the exact sums of the same samples in float64 (no ray stops, so every sample is composited): render()'s
    # outputs and the one call's are each held to the renderer's float bound against it
    sig64, raws64, dl64, _ = (x.double() for x in big)
    a64 = -torch.expm1(-sig64 * dl64) * (torch.arange(S, device=dev)[None, :] < n[:, None])
    T64 = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=torch.float64, device=dev), 1 - a64[:, :-1]], dim=1), dim=1)
    w64 = a64 * T64
    op64 = w64.sum(1).cpu().numpy()
    re64 = (w64[:, :, None] * raws64).sum(1).cpu().numpy()
    nc = n.cpu().numpy()
    vmax = big[1].abs().amax(dim=(0, 1)).cpu().numpy()
    assert (nc > 0).any() and float(re1[:, 3:].abs().max()) > 0
    for label, o_, norm_, sem_ in (("render()", r["opacity"], r["norm_nn"], r["sem"]),
                                   ("one composite call", op1, re1[:, 3:6], re1[:, 6:])):
        need = max(rc.bound_ratio(o_.cpu().numpy(), op64, nc, 1.0),
                   rc.bound_ratio(norm_.cpu().numpy(), re64[:, 3:6], nc, vmax[3:6]),
                   rc.bound_ratio(sem_.cpu().numpy(), re64[:, 6:], nc, vmax[6:]))
        print(f"heads at test time, {label} against the float64 sums: needs c = {need:.3f} (allowed {rc.GPU_C})")
        assert need <= rc.GPU_C, (label, need)


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
