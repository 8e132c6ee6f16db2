"""The geometry terms inside a captured step.  With loss_depth_w, loss_norm_depth_L1_w,
loss_norm_depth_dot_w and loss_reg_depth_w on, NeRFMTLoss reads nothing from the host: it can be
captured on its own with a device step counter, and Trainer(use_graph=True) runs in lockstep with the
eager Trainer across loss_norm_can_start.

Tolerances of the Trainer test: those of tests/test_gpu_graph.py for graph == eager (per-step loss
within 1e-4 relative; at most 5e-5 of the hash-table entries moved by more than 1e-4 and under 0.1 %
by more than 1e-6; MLP weights within 1e-3)."""
import numpy as np
import pytest
import torch

from ncnerf_amd.losses import NeRFMTLoss
from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
from ncnerf_amd.synthetic import SCENE_MAX, SCENE_MIN, SyntheticScene
from ncnerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
GEOM = dict(loss_depth_w=0.1, loss_norm_depth_L1_w=1e-3, loss_norm_depth_dot_w=1e-3, loss_reg_depth_w=1.0)
START = 500  # loss_norm_can_start of the Hypersim preset


def _labels(b, dev):
    """Depth and normal targets of a synthetic batch: the room's walls (the box the scene is built in)."""
    o, d = b["rays_o"].cpu().numpy(), b["rays_d"].cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (SCENE_MAX[None] - o) / d, (SCENE_MIN[None] - o) / d)
    t = np.where(np.isfinite(t) & (t > 0), t, np.inf)
    ax = t.argmin(axis=1)
    n = np.zeros_like(d)
    n[np.arange(len(ax)), ax] = -np.sign(d[np.arange(len(ax)), ax])
    depth = t.min(axis=1).astype(np.float32)
    depth[::7] = 0.0  # (masked labels)
    n[::5] = 0.0
    return torch.from_numpy(depth).to(dev), torch.from_numpy(n.astype(np.float32)).to(dev)


def _batches(dev, scene, n_rays, count, seed0):
    out = []
    for k in range(count):
        b = scene.torch_batch(n_rays, seed=seed0 + k, device=dev)
        b["march_noise"] = torch.rand(n_rays, device=dev, generator=torch.Generator(device=dev).manual_seed(k))
        b["depth"], b["normals"] = _labels(b, dev)
        out.append(b)
    return out


def test_loss_is_capturable(dev):
    """NeRFMTLoss with the four geometry terms, forward and backward, captured in a HIP graph with a
    device step counter: a host read inside it would fail the capture.  Replays at steps on both sides
    of loss_norm_can_start reproduce the eager module at the same host steps."""
    scene = SyntheticScene()
    b = _batches(dev, scene, 1024, 1, 90)[0]
    g = torch.Generator(device=dev).manual_seed(4)
    depth = (1.0 + 0.2 * torch.rand(1024, device=dev, generator=g)).requires_grad_(True)
    rgb = torch.rand(1024, 3, device=dev, generator=g).requires_grad_(True)
    pred = dict(rgb=rgb, depth=depth, opacity=torch.rand(1024, device=dev, generator=g), rays_o=b["rays_o"],
                rays_d=b["rays_d"])
    h = dict(GEOM, loss_opacity_w=0, loss_norm_can_start=START, ray_sampling_strategy="all_images_triang_patch",
             pred_norm_depth=True)
    loss = NeRFMTLoss(h)
    step_dev = torch.zeros((), dtype=torch.int64, device=dev)

    def body():
        ld = loss(pred, b, global_step=step_dev)
        (grad,) = torch.autograd.grad(ld["total"], depth)
        return ld, grad

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()  # (warm-up: the cached triangle indices are built outside the capture)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ld_g, grad_g = body()
    for step in (START - 1, START, START + 1, 3000):
        step_dev.fill_(step)
        graph.replay()
        torch.cuda.synchronize()
        ld_e = loss(pred, b, global_step=step)
        (grad_e,) = torch.autograd.grad(ld_e["total"], depth)
        torch.cuda.synchronize()
        assert set(ld_g) == {"rgb", "depth", "norm_D_L1", "norm_D_dot", "reg_depth", "total"}
        assert set(ld_e) == set(ld_g) - (set() if step > START else {"reg_depth"})
        for k in ("depth", "norm_D_L1", "norm_D_dot"):
            assert float(ld_g[k]) == float(ld_e[k]) != 0.0, (step, k)  # (fixed-order sums: the same bits)
        if step > START:
            assert float(ld_g["reg_depth"]) == float(ld_e["reg_depth"]) > 0.0
        else:
            assert float(ld_g["reg_depth"]) == 0.0
        # (the triangle scatters are float atomics: equal up to summation order)
        assert float((grad_g - grad_e).norm() / grad_e.norm()) < 1e-5, step


def _model(dev, scene, seed=7):
    torch.manual_seed(seed)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-1e-2, 1e-2)
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    return m


def test_graph_trainer_with_geometry_terms_matches_eager(dev):
    """Trainer(use_graph=True) with depth and normal supervision on a 1024-ray batch with targets,
    global steps 499 .. 502 (the RegNeRF term starts after 500), against the eager Trainer."""
    scene = SyntheticScene()
    batches = _batches(dev, scene, 1024, 4, 50)
    losses, params, keys = [], [], []
    for use_graph in (False, True):
        m = _model(dev, scene)
        tr = Trainer(m, hparams=dict(GEOM), update_grid=False, use_graph=use_graph)
        ls = []
        for k, b in enumerate(batches):
            _, ld = tr.step(b, global_step=START - 1 + k)
            ls.append([float(ld[q]) for q in ("total", "depth", "norm_D_L1", "norm_D_dot")]
                      + [float(ld["reg_depth"]) if "reg_depth" in ld else 0.0])
            keys.append(set(ld))
        torch.cuda.synchronize()
        losses.append(np.array(ls))
        params.append(m.flat_params().detach().clone())
    assert all({"depth", "norm_D_L1", "norm_D_dot", "norm_D_C_ort_dot", "rgb", "opacity"} <= k for k in keys)
    assert (losses[0][:, 1:4] > 0).all() and (losses[1][:, 1:4] > 0).all()
    # the RegNeRF term: absent (eager) / 0 (graph) at steps 499 and 500, on at 501 and 502
    assert (losses[0][:2, 4] == 0).all() and (losses[1][:2, 4] == 0).all() and (losses[1][2:, 4] > 0).all()
    np.testing.assert_allclose(losses[1], losses[0], rtol=1e-4)
    n_t = m._n_table
    d = (params[1][:n_t] - params[0][:n_t]).abs()
    assert int((d > 1e-4).sum()) <= 5e-5 * n_t, int((d > 1e-4).sum())
    assert float((d > 1e-6).float().mean()) < 1e-3
    rel_w = float((params[1][n_t:] - params[0][n_t:]).norm() / params[0][n_t:].norm())
    assert rel_w < 1e-3, rel_w
