"""Camera pose refinement (the reference's --optimize_ext, train_nerf.py:177-180, 244-249): rays that
require grad get their gradient through every stage.

Normals: rays_o.grad, rays_d.grad and depth.grad of `_Normals` (ncn_normals_bwd_rays) against torch
autograd through oracle.losses_ref.normals_from_depth, rel-L2 <= 1e-4 (the existing d depth bound of
tests/test_gpu_loss.py), with rays_o a separate leaf and with rays_o the same tensor as rays_d
(render()'s quirk q1: results['rays_o'] = rays_d).

End to end: 128 rays of a pose with leaf dR (axis-angle) and dT through RayMarcher.apply (dynamic
shapes, injected noise) -> NGPMT -> VolumeRenderer.apply -> photometric + normals loss.  The ray
gradients equal the fp64 segment sums of the retained dL/dxyzs, dL/ddirs (RayMarcher.backward,
custom_functions.py:102-112) plus the normals' own ray term within the summation-order bound of the
segment sum, 2 n 2^-24 sum|terms| (n samples + the normals term: n + 1 addends), plus the f32-atomics
order of the normals term itself, 2 (6 - 1) 2^-24 sum|corner contributions| (a ray is a corner of at
most 6 triangles).  The same rays through render() + NeRFMTLoss with the clustering on reach the
pose through the unfused loss branch; the static-shape path and the fused loss nodes refuse rays
that require grad instead of dropping the gradient."""
import numpy as np
import pytest
import torch

from ncnerf_amd import losses as L
from ncnerf_amd import vren
from ncnerf_amd.custom_functions import RayMarcher, VolumeRenderer
from ncnerf_amd.ngp_mt import NGPMT
from ncnerf_amd.rendering import render
from ncnerf_amd.synthetic import SyntheticScene
from ncnerf_amd.trainer import HYPERSIM_HPARAMS
from oracle import losses_ref

pytestmark = pytest.mark.gpu

R = 128
U = 2.0 ** -24


def _triangles(dev=None):
    x1, x2, x3 = losses_ref.patch_triangle_index(R)
    assert len(x1) == 98
    if dev is None:
        return x1, x2, x3
    return {k: torch.from_numpy(v).to(dev) for k, v in zip(("x1", "x2", "x3"), (x1, x2, x3))}


def _rel(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("shared", [False, True], ids=["o_leaf", "o_is_d"])
def test_normals_ray_gradients(dev, shared):
    rng = np.random.default_rng(5)
    d = rng.normal(size=(R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = rng.normal(size=(R, 3)).astype(np.float32) * 0.3
    depth = rng.uniform(0.5, 2.0, R).astype(np.float32)
    gn = torch.from_numpy(rng.normal(size=(98, 3)).astype(np.float32))
    x1, x2, x3 = _triangles()
    # reference: torch autograd on the host
    dr = torch.from_numpy(d).requires_grad_(True)
    orr = dr if shared else torch.from_numpy(o).requires_grad_(True)
    zr = torch.from_numpy(depth).requires_grad_(True)
    (losses_ref.normals_from_depth(orr, dr, zr, x1, x2, x3) * gn).sum().backward()
    # device
    dd = torch.from_numpy(d).to(dev).requires_grad_(True)
    od = dd if shared else torch.from_numpy(o).to(dev).requires_grad_(True)
    zd = torch.from_numpy(depth).to(dev).requires_grad_(True)
    n = L.extract_normals_from_ray_batch(od, dd, zd, _triangles(dev))
    (n * gn.to(dev)).sum().backward()
    errs = {"rays_d": _rel(dd.grad, dr.grad), "depth": _rel(zd.grad, zr.grad)}
    if not shared:
        errs["rays_o"] = _rel(od.grad, orr.grad)
    print("normals ray gradients rel-L2:", "o is d" if shared else "o leaf", errs)
    assert all(e <= 1e-4 for e in errs.values()), errs


def test_fused_loss_nodes_refuse_ray_gradients(dev):
    rng = np.random.default_rng(6)
    d = torch.from_numpy(rng.normal(size=(R, 3)).astype(np.float32)).to(dev).requires_grad_(True)
    depth = torch.from_numpy(rng.uniform(0.5, 2.0, R).astype(np.float32)).to(dev).requires_grad_(True)
    with pytest.raises(RuntimeError, match="rays_o / rays_d"):
        L.normals_cluster_losses(d, d, depth, _triangles(dev))


def _axis_angle(w):
    """Rodrigues: exp of the skew matrix of w (3,), |w| > 0."""
    theta = w.norm()
    k = w / theta
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    K = torch.stack([torch.stack([z, -k[2], k[1]]), torch.stack([k[2], z, -k[0]]), torch.stack([-k[1], k[0], z])])
    return torch.eye(3, dtype=w.dtype, device=w.device) + torch.sin(theta) * K + (1 - torch.cos(theta)) * (K @ K)


@pytest.fixture(scope="module")
def setup(dev):
    scene = SyntheticScene()
    batch = scene.torch_batch(R, seed=1, device=dev)
    torch.manual_seed(0)
    m = NGPMT(scale=0.5, grid_size=128).to(dev)
    m.amp_state[0] = 1.0  # (upstream gradients of order 1e-3: no need for the GradScaler's 2^16)
    m.density_bitfield.fill_(255)  # every occupancy bit set
    noise = torch.rand(R, generator=torch.Generator().manual_seed(3)).to(dev)
    return m, batch, noise


def _posed_rays(batch, dev):
    dR = torch.tensor([0.01, -0.02, 0.015], device=dev, requires_grad=True)
    dT = torch.tensor([0.002, -0.001, 0.003], device=dev, requires_grad=True)
    rays_d = batch["rays_d"] @ _axis_angle(dR).T
    rays_o = batch["rays_o"] + dT
    return dR, dT, rays_o, rays_d


def test_pose_gradient_end_to_end(dev, setup):
    m, batch, noise = setup
    m.flat_grad().zero_()
    dR, dT, rays_o, rays_d = _posed_rays(batch, dev)
    rays_o.retain_grad()
    rays_d.retain_grad()
    _, hits_t, _ = vren.ray_aabb_intersect(rays_o.detach().contiguous(), rays_d.detach().contiguous(), m.center,
                                           m.half_size, 1, near_distance=0.01)
    rays_a, xyzs, dirs, deltas, ts, total = RayMarcher.apply(rays_o, rays_d, hits_t[:, 0], m.density_bitfield,
                                                             m.cascades, m.scale, 0.0, m.grid_size, 256, noise, False)
    S = int(total)
    assert xyzs.shape[0] == S and S > R
    xyzs.retain_grad()
    dirs.retain_grad()
    out = m(xyzs, dirs)
    _, opacity, depth, rend, _ = VolumeRenderer.apply(out["sigmas"], out["rgbs"], deltas, ts, rays_a, 1e-4)
    tri = _triangles(dev)
    gn = torch.randn(98, 3, generator=torch.Generator().manual_seed(4)).to(dev) * 1e-3
    normals = L.extract_normals_from_ray_batch(rays_o, rays_d, depth, tri)
    loss = ((rend - batch["rgb"]) ** 2).mean() + (normals * gn).sum()
    loss.backward()
    for t in (dR.grad, dT.grad, rays_o.grad, rays_d.grad, xyzs.grad, dirs.grad):
        assert t is not None and bool(torch.isfinite(t).all())
    assert float(dR.grad.abs().max()) > 0 and float(dT.grad.abs().max()) > 0
    assert float(xyzs.grad.abs().max()) > 0 and float(dirs.grad.abs().max()) > 0
    # the normals' own ray term, evaluated on the device again (the same f32 corner contributions;
    # only their atomics order may differ), and the corner contributions' absolute sums on the host
    o2, d2 = rays_o.detach().clone().requires_grad_(True), rays_d.detach().clone().requires_grad_(True)
    (L.extract_normals_from_ray_batch(o2, d2, depth.detach(), tri) * gn).sum().backward()
    x1, x2, x3 = (torch.from_numpy(v) for v in _triangles())
    oc, dc, zc = rays_o.detach().cpu().double(), rays_d.detach().cpu().double(), depth.detach().cpu().double()
    Pc = oc + dc * zc[:, None]
    corners = [Pc[i].clone().requires_grad_(True) for i in (x1, x2, x3)]
    nref = torch.nn.functional.normalize(torch.cross(corners[1] - corners[0], corners[2] - corners[0], dim=-1), dim=-1)
    (nref * gn.cpu().double()).sum().backward()
    abs_o, abs_d = torch.zeros(R, 3, dtype=torch.float64), torch.zeros(R, 3, dtype=torch.float64)
    for i, c in zip((x1, x2, x3), corners):
        abs_o.index_add_(0, i, c.grad.abs())
        abs_d.index_add_(0, i, c.grad.abs() * zc[i][:, None])
    # fp64 segment sums of the retained gradients (rows are rays: rays_a[i] = (ray, start, count))
    gx, gd, t64 = xyzs.grad.cpu().double(), dirs.grad.cpu().double(), ts.detach().cpu().double()
    term_d = gx * t64[:, None] + gd
    worst = 0.0
    for ray, s0, cnt in rays_a.cpu().tolist():
        seg = slice(s0, s0 + cnt)
        for got, terms, nterm, ab in ((rays_o.grad, gx[seg], o2.grad, abs_o), (rays_d.grad, term_d[seg], d2.grad, abs_d)):
            nt = nterm[ray].cpu().double()
            ref = terms.sum(0) + nt
            bound = 2.0 * cnt * U * (terms.abs().sum(0) + nt.abs()) * 1.01 + 2.0 * 5 * U * ab[ray] * 1.01 + 1e-30
            err = (got[ray].cpu().double() - ref).abs()
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), (ray, err, bound)
    print(f"pose gradient: S = {S}, worst ray-gradient error / bound = {worst:.3f}, "
          f"|dR.grad| = {float(dR.grad.norm()):.3e}, |dT.grad| = {float(dT.grad.norm()):.3e}")


def test_render_and_loss_reach_the_pose(dev, setup):
    m, batch, noise = setup
    m.flat_grad().zero_()
    dR, dT, rays_o, rays_d = _posed_rays(batch, dev)
    kw = dict(near_distance=0.01, max_samples=256, test_time=False, random_bg=False, anneal_strategy="none",
              anneal_steps=0, march_noise=noise, global_step=3000)
    loss = L.NeRFMTLoss(dict(HYPERSIM_HPARAMS))
    res = render(m, rays_o, rays_d, **kw)
    assert res["rays_o"] is res["rays_d"] and res["rays_d"].requires_grad  # (quirk q1)
    loss_d = loss(res, batch, global_step=3000)
    # the unfused branch: the fused node would have kept the normals it saw (and refuses such rays)
    assert loss.last_normals is None and loss.last_cluster is not None
    assert "norm_D_C_ort_dot" in loss_d
    loss_d["total"].backward()
    assert bool(torch.isfinite(dR.grad).all()) and float(dR.grad.abs().max()) > 0
    assert bool(torch.isfinite(dT.grad).all()) and float(dT.grad.abs().max()) > 0
    print(f"render + NeRFMTLoss: |dR.grad| = {float(dR.grad.norm()):.3e}, |dT.grad| = {float(dT.grad.norm()):.3e}")


def test_static_shapes_refuse_ray_gradients(dev, setup):
    m, batch, noise = setup
    _, _, rays_o, rays_d = _posed_rays(batch, dev)
    with pytest.raises(RuntimeError, match="require grad"):
        render(m, rays_o, rays_d, near_distance=0.01, max_samples=256, test_time=False, march_noise=noise,
               static_shapes=True)
