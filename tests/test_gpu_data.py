"""The device data path (ncnerf_amd.data: ncn_batch_draw, ncn_batch_rays_fw, ncn_batch_rays_bw)
against the host restatement tests/data_ref.py.

Bounds (u = 2^-24):
* draws: bit-identical to the restatement (integers);
* forward, stored poses: rgb and rays_o exact; rays_d within the 3-term order bound
  2 u sum_j |R_ij dir_j| of the fp64 product;
* forward with dR / dT: rays_d within 16 u |dir| per component of the fp64 formula (two 3-term
  products at 2 u sqrt(3) |dir| each plus four ulp for the coefficients, rounded up); at |dR| = 0.02 a
  transposed or swapped product or a wrong sign moves a component by ~1e-2 |dir|; rays_o = fl(t + dT);
* backward: rel-L2 <= 1e-4 against fp64 autograd through the restated formula (the bound of
  tests/test_gpu_pose_grad.py for fp32 gradient kernels); absent images exactly zero; two runs
  bit-identical."""
import numpy as np
import pytest
import torch

import data_ref
from ncnerf_amd import data as D
from ncnerf_amd.data import DeviceRayDataset
from ncnerf_amd.losses import NeRFMTLoss
from ncnerf_amd.ngp_mt import NGPMT
from ncnerf_amd.rendering import render
from ncnerf_amd.synthetic import make_cameras
from ncnerf_amd.trainer import HYPERSIM_HPARAMS

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (V, H, W, patch, rays): 5 images of 24x20; one image with two corners; area 16 (4 patches per wave)
SHAPES = {"v5_p8": (5, 20, 24, 8, 1024), "v1_two_corners": (1, 8, 9, 8, 64), "v5_p4": (5, 20, 24, 4, 256)}
STEPS = (0, 1, 2 ** 32 + 3)


def _rel(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


# ---- draw ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("corner_mode", ["reference", "grid"])
@pytest.mark.parametrize("same_image", [False, True], ids=["all_images", "same_image"])
def test_draw_is_the_restatement(dev, shape, corner_mode, same_image):
    V, H, W, p, R = SHAPES[shape]
    n_p = R // (p * p)
    for seed in (0, 2 ** 63 + 5):
        for step in STEPS:
            ref_i, ref_p = data_ref.draw(seed, step, V, H, W, p, n_p, same_image, corner_mode)
            assert 0 <= ref_p.min() and ref_p.max() < H * W
            for s in (step, torch.tensor(step, dtype=torch.int64, device=dev)):  # host value / device counter
                img = torch.full((R,), -1, dtype=torch.int64, device=dev)
                pix = torch.full((R,), -1, dtype=torch.int64, device=dev)
                D.batch_draw(seed, s, V, H, W, p, n_p, same_image, D.CORNER_MODES[corner_mode], img, pix)
                assert np.array_equal(img.cpu().numpy(), ref_i), (seed, step)
                assert np.array_equal(pix.cpu().numpy(), ref_p), (seed, step)
            if same_image:
                assert len(set(ref_i.tolist())) == 1


def test_draw_refuses_bad_arguments(dev):
    from ncnerf_amd._lib import NcnError
    img = torch.zeros(64, dtype=torch.int64, device=dev)
    with pytest.raises(NcnError, match="does not fit"):
        D.batch_draw(0, 0, 1, 8, 7, 8, 1, False, 0, img, img.clone())
    with pytest.raises(NcnError, match="corner_mode"):
        D.batch_draw(0, 0, 1, 8, 8, 8, 1, False, 2, img, img.clone())


# ---- forward ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene5(dev):
    V, H, W, p, R = SHAPES["v5_p8"]
    images, poses, directions = data_ref.small_scene(V, H, W, seed=1)
    img, pix = data_ref.draw(9, 4, V, H, W, p, R // (p * p))
    host = dict(images=images, poses=torch.from_numpy(poses), directions=torch.from_numpy(directions),
                img=torch.from_numpy(img), pix=torch.from_numpy(pix))
    d = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).to(dev) for k, v in host.items()}
    return host, d


def _forward(d, images, dR=None, dT=None):
    R = d["img"].numel()
    o, dd, rgb = (torch.full((R, 3), float("nan"), device=d["img"].device) for _ in range(3))
    D.batch_rays_fw(d["img"], d["pix"], images, d["directions"], d["poses"], dR, dT, o, dd, rgb)
    return o.cpu(), dd.cpu(), rgb.cpu()


@pytest.mark.parametrize("storage", ["uint8", "float32"])
def test_forward_with_stored_poses(dev, scene5, storage):
    host, d = scene5
    if storage == "uint8":
        images = d["images"]
        rgb_ref = host["images"][host["img"].numpy(), host["pix"].numpy()].astype(np.float32) / np.float32(255.0)
    else:
        f = np.random.default_rng(2).random(host["images"].shape, dtype=np.float32)
        images = torch.from_numpy(f).to(dev)
        rgb_ref = f[host["img"].numpy(), host["pix"].numpy()]
    o, dd, rgb = _forward(d, images)
    assert np.array_equal(rgb.numpy(), rgb_ref)
    P = host["poses"][host["img"]]
    assert torch.equal(o, P[:, :, 3])
    terms = P[:, :, :3].double() * host["directions"][host["pix"]].double()[:, None, :]  # (R, i, j)
    err = (dd.double() - terms.sum(-1)).abs()
    bound = 2 * U * terms.abs().sum(-1)
    print(f"rays_d, stored poses: worst error / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def _pose_params(V, mag, seed):
    """dR (V,3) of norm `mag` about different (non-commuting) axes, dT ~ 1e-3."""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=(V, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    return torch.from_numpy((mag * ax).astype(np.float32)), torch.from_numpy(
        rng.uniform(-2e-3, 2e-3, size=(V, 3)).astype(np.float32))


@pytest.mark.parametrize("mag", [0.0, 1e-6, 0.02])
def test_forward_with_pose_corrections(dev, scene5, mag):
    host, d = scene5
    dR, dT = _pose_params(5, mag, seed=3)
    o, dd, rgb = _forward(d, d["images"], dR.to(dev), dT.to(dev))
    o_ref, d_ref = data_ref.rays(host["poses"], host["directions"], host["img"], host["pix"], dR.double(), dT.double())
    assert torch.equal(o, host["poses"][host["img"]][:, :, 3] + dT[host["img"]])  # fl(t + dT)
    norm = host["directions"][host["pix"]].double().norm(dim=1, keepdim=True)
    err = (dd.double() - d_ref).abs()
    print(f"rays_d, |dR| = {mag}: worst error / (16 u |dir|) = {float((err / (16 * U * norm)).max()):.3f}")
    assert bool((err <= 16 * U * norm).all())
    if mag == 0.02:  # the correction is far above the bound: a wrong product order would not pass
        _, plain = data_ref.rays(host["poses"], host["directions"], host["img"], host["pix"])
        assert float((d_ref - plain).abs().max()) > 1e3 * 16 * U


def test_forward_flags_indices_out_of_range(dev, scene5):
    host, d = scene5
    bad = dict(d, img=d["img"].clone(), pix=d["pix"].clone())
    bad["img"][3], bad["pix"][5], bad["pix"][7] = 5, 20 * 24, -1
    o, dd, rgb = _forward(bad, d["images"])
    nan_rows = torch.isnan(dd).any(1)
    assert nan_rows.nonzero().flatten().tolist() == [3, 5, 7]
    assert bool(torch.isnan(o[nan_rows]).all()) and bool(torch.isnan(rgb[nan_rows]).all())


# ---- backward --------------------------------------------------------------------------------
def _backward_case(dev, host, d, img, pix, mag, seed):
    """Device grad_dR / grad_dT (buffers NaN beforehand) and the fp64 autograd reference."""
    V = host["poses"].shape[0]
    R = img.numel()
    g = torch.Generator().manual_seed(seed)
    g_o, g_d = torch.randn(R, 3, generator=g), torch.randn(R, 3, generator=g)
    dR, dT = _pose_params(V, mag, seed=seed)
    dR64, dT64 = dR.double().requires_grad_(True), dT.double().requires_grad_(True)
    o_ref, d_ref = data_ref.rays(host["poses"], host["directions"], img, pix, dR64, dT64)
    ((o_ref * g_o.double()).sum() + (d_ref * g_d.double()).sum()).backward()
    outs = []
    for _ in range(2):
        gR = torch.full((V, 3), float("nan"), device=dev)
        gT = torch.full((V, 3), float("nan"), device=dev)
        D.batch_rays_bw(g_o.to(dev), g_d.to(dev), img.to(dev), pix.to(dev), d["directions"], d["poses"], dR.to(dev),
                        gR, gT)
        outs.append((gR.cpu(), gT.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])  # no atomics
    return outs[0][0], outs[0][1], dR64.grad, dT64.grad


@pytest.mark.parametrize("mag", [0.0, 1e-6, 0.02])
def test_backward_matches_fp64_autograd(dev, scene5, mag):
    host, d = scene5
    gR, gT, rR, rT = _backward_case(dev, host, d, host["img"], host["pix"], mag, seed=11)
    assert bool(torch.isfinite(rR).all()) and float(rR.abs().min()) > 0
    errs = {"dR": _rel(gR, rR), "dT": _rel(gT, rT)}
    print(f"pose backward, |dR| = {mag}: rel-L2 {errs}")
    assert all(e <= 1e-4 for e in errs.values()), errs


@pytest.mark.parametrize("shape", ["v5_p4", "v1_two_corners"])
def test_backward_small_patches(dev, shape):
    V, H, W, p, R = SHAPES[shape]
    images, poses, directions = data_ref.small_scene(V, H, W, seed=4)
    host = dict(poses=torch.from_numpy(poses), directions=torch.from_numpy(directions))
    d = {k: v.to(dev) for k, v in host.items()}
    img, pix = (torch.from_numpy(x) for x in data_ref.draw(2, 1, V, H, W, p, R // (p * p)))
    gR, gT, rR, rT = _backward_case(dev, host, d, img, pix, 0.02, seed=12)
    present = torch.zeros(V, dtype=torch.bool)
    present[img] = True
    assert _rel(gR[present], rR[present]) <= 1e-4 and _rel(gT[present], rT[present]) <= 1e-4
    assert bool((gR[~present] == 0).all()) and bool((gT[~present] == 0).all())


def test_backward_interleaved_and_absent_images(dev, scene5):
    """Rays of the images {0, 2, 3} in random order (no runs of a patch): rows 1 and 4 are exactly zero."""
    host, d = scene5
    g = torch.Generator().manual_seed(5)
    img = torch.tensor([0, 2, 3])[torch.randint(0, 3, (1000,), generator=g)]
    pix = torch.randint(0, 20 * 24, (1000,), generator=g)
    gR, gT, rR, rT = _backward_case(dev, host, d, img, pix, 0.02, seed=13)
    for got, ref in ((gR, rR), (gT, rT)):
        assert bool((got[[1, 4]] == 0).all()) and bool((ref[[1, 4]] == 0).all())
        assert _rel(got, ref) <= 1e-4


# ---- dataset -----------------------------------------------------------------------------------
def _room_dataset(dev, batch_size, **kw):
    """5 cameras inside the synthetic room, 24x20 images: every ray marches into the walls."""
    V, H, W = 5, 20, 24
    images, _, directions = data_ref.small_scene(V, H, W, seed=6)
    poses = make_cameras(V, seed=2)
    return DeviceRayDataset(torch.from_numpy(images).to(dev), torch.from_numpy(poses).to(dev),
                            torch.from_numpy(directions).to(dev), (W, H), batch_size=batch_size, seed=21, **kw)


def test_dataset_batch_and_image_rays(dev):
    ds = _room_dataset(dev, 1024, ray_sampling_strategy="same_image_triang_patch", corner_mode="grid")
    b = ds.batch(torch.tensor(5, dtype=torch.int64, device=dev))
    ref_i, ref_p = data_ref.draw(21, 5, 5, 20, 24, 8, 16, True, "grid")
    assert np.array_equal(b["img_idxs"].cpu().numpy(), ref_i) and np.array_equal(b["pix_idxs"].cpu().numpy(), ref_p)
    assert b["patch_area"] == 64 and len(b["x1_offsets_local"]) == 49
    v = int(ref_i[0])
    o, dd, rgb = ds.image_rays(v)
    assert o.shape == dd.shape == rgb.shape == (480, 3)
    assert torch.equal(dd[b["pix_idxs"]], b["rays_d"]) and torch.equal(rgb[b["pix_idxs"]], b["rgb"])
    assert torch.equal(o[b["pix_idxs"]], b["rays_o"])
    assert np.array_equal(rgb.cpu().numpy(), ds.images[v].cpu().numpy().astype(np.float32) / np.float32(255.0))
    # rank r of a data-parallel run draws with seed + r
    assert not torch.equal(ds.batch(5, seed=22)["pix_idxs"], b["pix_idxs"])


def test_pose_gradients_through_the_dataset(dev):
    """128 rays of an optimize_ext dataset through render + NeRFMTLoss (the eager dynamic-shape path of
    tests/test_gpu_pose_grad.py): dR.grad / dT.grad are ncn_batch_rays_bw of the ray gradients bit for
    bit, and the fp64 chain of those ray gradients within 1e-4."""
    ds = _room_dataset(dev, 128, optimize_ext=True)
    torch.manual_seed(0)
    m = NGPMT(scale=0.5, grid_size=128).to(dev)
    m.amp_state[0] = 1.0  # (as tests/test_gpu_pose_grad.py: upstream gradients of order 1e-3)
    m.density_bitfield.fill_(255)
    with torch.no_grad():  # start from a pose correction that is not the origin
        dR0, dT0 = _pose_params(5, 0.02, seed=8)
        ds.dR.copy_(dR0.to(dev))
        ds.dT.copy_(dT0.to(dev))
    step = 3000
    loss = NeRFMTLoss(dict(HYPERSIM_HPARAMS))
    noise = torch.rand(128, generator=torch.Generator().manual_seed(3)).to(dev)
    kw = dict(near_distance=0.01, max_samples=256, test_time=False, random_bg=False, anneal_strategy="none",
              anneal_steps=0, march_noise=noise, global_step=step)

    def run(rays_o, rays_d, batch):
        m.flat_grad().zero_()
        loss_d = loss(render(m, rays_o, rays_d, **kw), batch, global_step=step)
        loss_d["total"].backward()

    # through the dataset's Function; the ray gradients that reach it are retained in the same pass
    b = ds.batch(step)
    assert b["rays_d"].requires_grad and not b["rgb"].requires_grad
    b["rays_o"].retain_grad()
    b["rays_d"].retain_grad()
    run(b["rays_o"], b["rays_d"], b)
    g_o = b["rays_o"].grad if b["rays_o"].grad is not None else torch.zeros_like(b["rays_d"])
    g_d = b["rays_d"].grad
    assert bool(torch.isfinite(ds.dR.grad).all()) and float(ds.dR.grad.abs().max()) > 0
    gR, gT = torch.empty_like(ds.dR), torch.empty_like(ds.dT)
    D.batch_rays_bw(g_o, g_d, b["img_idxs"], b["pix_idxs"], ds.directions, ds.poses, ds.dR.detach(), gR, gT)
    assert torch.equal(gR, ds.dR.grad) and torch.equal(gT, ds.dT.grad)  # same inputs, deterministic kernel
    # the fp64 chain of those ray gradients
    dR64 = ds.dR.detach().cpu().double().requires_grad_(True)
    dT64 = ds.dT.detach().cpu().double().requires_grad_(True)
    o_ref, d_ref = data_ref.rays(ds.poses.cpu(), ds.directions.cpu(), b["img_idxs"].cpu(), b["pix_idxs"].cpu(), dR64, dT64)
    ((o_ref * g_o.cpu().double()).sum() + (d_ref * g_d.cpu().double()).sum()).backward()
    errs = {"dR": _rel(ds.dR.grad, dR64.grad), "dT": _rel(ds.dT.grad, dT64.grad)}
    print(f"pose gradients through the dataset vs the fp64 chain: rel-L2 {errs}")
    assert all(e <= 1e-4 for e in errs.values()), errs
    # the same rays as detached leaves: their gradients (equal up to the order of the loss
    # backward's float atomics) through the kernel give the same pose gradients
    lo, ld = b["rays_o"].detach().clone().requires_grad_(True), b["rays_d"].detach().clone().requires_grad_(True)
    run(lo, ld, dict(b, rays_o=lo, rays_d=ld))
    l_o = lo.grad if lo.grad is not None else torch.zeros_like(ld)
    D.batch_rays_bw(l_o, ld.grad, b["img_idxs"], b["pix_idxs"], ds.directions, ds.poses, ds.dR.detach(), gR, gT)
    same_inputs = torch.equal(l_o, g_o) and torch.equal(ld.grad, g_d)
    leaf = {"dR": _rel(gR, ds.dR.grad.cpu()), "dT": _rel(gT, ds.dT.grad.cpu()), "same ray gradients": same_inputs,
            "bit-identical": torch.equal(gR, ds.dR.grad) and torch.equal(gT, ds.dT.grad)}
    print(f"pose gradients from the detached-leaf run vs the Function's: {leaf}")
    assert leaf["dR"] <= 1e-4 and leaf["dT"] <= 1e-4
    assert leaf["bit-identical"] or not same_inputs  # same inputs, deterministic kernel
