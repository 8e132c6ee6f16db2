"""The geometry terms of NeRFMTLoss on the device (ncn_geom_loss_fwd / _bwd): depth L2, GT-normal
L1 / dot, RegNeRF, with the validity filter.

References and bounds:
 * every case of tests/golden/geom_losses.npz (the reference's own NeRFMTLoss.forward in float64), through
   NeRFMTLoss on the device; the kernel-level shapes against the float64 restatement of tests/geom_ref.py,
   which tests/test_geom_host.py holds to that fixture;
 * a loss within the fixed-order bound of its float64 value: 2 (n - 1) 2^-24 sum|addends| times the
   mean's factor (weight / count), n the number of addends of the mean;
 * d loss / d depth (and d loss / d normals) within 1e-4 (rel. L2) of float64, the bound of
   tests/test_gpu_pose_grad.py for float32 gradient kernels;
 * a filtered term, an empty mask: exactly 0 loss, exactly zero finite gradient;
 * two runs of the forward, and of the depth term's backward, are bit-identical.
"""
import os

import numpy as np
import pytest
import torch

import geom_ref
from geom_ref import KEYS, fixed_order_bound
from ncnerf_amd import losses
from ncnerf_amd.losses import (GEOM_DEPTH, GEOM_NORM_DOT, GEOM_NORM_L1, GEOM_REG, NeRFMTLoss,
                               extract_normals_from_ray_batch, geometry_losses)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("depth", "norm", "norm_gtdepth", "reg_off", "reg_on", "all", "empty", "nan")
GRAD_BOUND = 1e-4
ALL = GEOM_DEPTH | GEOM_NORM_L1 | GEOM_NORM_DOT | GEOM_REG
W = (0.1, 0.05, 0.02)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "geom_losses.npz"))


def rel_l2(got, want):
    return float((got.double().cpu() - want.double()).norm() / want.double().norm())


def run_module(case, dev, step):
    """NeRFMTLoss of the case on the device -> (loss_d, d total / d depth)."""
    f = lambda t: t.float().to(dev)
    depth = f(case.depth).requires_grad_(True)
    R = depth.shape[0]
    pred = dict(rgb=f(case.rgb_pred).requires_grad_(True), depth=depth, opacity=torch.zeros(R, device=dev),
                rays_o=f(case.rays_o), rays_d=f(case.rays_d))
    target = dict(rgb=f(case.rgb_gt), depth=f(case.depth_gt), normals=f(case.normals),
                  normals_depth=f(case.normals_depth))
    if case.offsets is not None:
        target.update(patch_area=64, x1_offsets_local=case.offsets[0], x2_offsets_local=case.offsets[1],
                      x3_offsets_local=case.offsets[2])
    ld = NeRFMTLoss(case.hparams())(pred, target, global_step=step)
    ld["total"].backward()
    torch.cuda.synchronize()
    # (no geometry term in the graph, the RegNeRF term before its start with a host step: no gradient at all)
    return ld, (torch.zeros_like(depth) if depth.grad is None else depth.grad)


def check_against(case, ld, grad, keys):
    terms, _ = case.restated()  # float64: the addends of each mean
    for k in sorted(keys):
        got = float(ld[k])
        want = case.loss64.get(k, case.loss64.get("norm", 0.0) if k.startswith("norm_D") else 0.0)
        bound = fixed_order_bound(terms[k][1], terms[k][2]) if k in terms and want != 0.0 else 0.0
        print(f"{k}: got {got!r} float64 {want!r} |diff| {abs(got - want):.3e} bound {bound:.3e}")
        assert abs(got - want) <= bound, (k, got, want, bound)
    want = torch.from_numpy(case.grad64)
    assert bool(torch.isfinite(grad).all())
    if not case.grad64.any():
        assert not bool(grad.any())
    else:
        err = rel_l2(grad, want)
        print(f"d total / d depth: rel. L2 {err:.3e}")
        assert err <= GRAD_BOUND, err


@pytest.mark.parametrize("tag", ["tri", "patch"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_case(dev, golden, tag, name):
    case = geom_ref.FixtureCase(golden, tag, name)
    ld, grad = run_module(case, dev, case.step)
    assert set(ld) - {"rgb", "total"} == case.expected_keys()
    check_against(case, ld, grad, case.expected_keys())
    if case.variant in ("empty", "nan"):
        assert all(float(ld[k]) == 0.0 for k in case.expected_keys())
        assert float(ld["total"]) == float(ld["rgb"])


@pytest.mark.parametrize("name", ["reg_off", "reg_on", "all", "nan"])
def test_device_step_is_the_host_step(dev, golden, name):
    """A device int64 global_step: the RegNeRF gate is taken by the kernel.  The entry is then always
    there, 0 with zero gradient until step > loss_norm_can_start; everything else as with the host step."""
    case = geom_ref.FixtureCase(golden, "patch", name)
    ld, grad = run_module(case, dev, torch.tensor(case.step, dtype=torch.int64, device=dev))
    assert set(ld) - {"rgb", "total"} == case.expected_keys() | {"reg_depth"}
    check_against(case, ld, grad, case.expected_keys() | {"reg_depth"})
    if name == "reg_off":
        assert float(ld["reg_depth"]) == 0.0 and not bool(grad.any())


# ---- the kernels' shapes ----
_INPUTS = {}


def node_inputs(n_patches):
    """Patches of well-conditioned rays (geom_ref.patch_rays) with noisy depths, depth labels with
    zeros, GT normals with zero rows and free predicted normals: CPU float32 tensors, built once."""
    if n_patches not in _INPUTS:
        rng = np.random.default_rng(100 + n_patches)
        o, d = geom_ref.patch_rays(rng, n_patches)
        true_depth, n = geom_ref.box_exit(o, d)
        R = len(true_depth)
        depth = (true_depth * (1 + 0.01 * rng.standard_normal(R))).astype(np.float32)
        depth_gt = (true_depth * (1 + 0.002 * rng.standard_normal(R))).astype(np.float32)
        depth_gt[rng.random(R) < 0.2] = 0.0
        normals_gt = (n + 0.1 * rng.standard_normal((R, 3))).astype(np.float32)
        normals_gt[rng.random(R) < 0.25] = 0.0
        x = geom_ref.triangles(R, "all_images_triang_patch")
        free = rng.standard_normal((x["x1"].numel(), 3)).astype(np.float32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        _INPUTS[n_patches] = dict(rays_o=t(o), rays_d=t(d), depth=t(depth), depth_gt=t(depth_gt),
                                  normals_gt=t(normals_gt), free_normals=t(free), x=x)
    return _INPUTS[n_patches]


def reference64(inp, through_rays):
    """float64 terms and gradients of the restatement: (terms, d/d depth, d/d normals or None)."""
    d64 = lambda k: inp[k].double()
    depth = d64("depth").requires_grad_(True)
    if through_rays:
        normals = geom_ref.extract_normals(d64("rays_o"), d64("rays_d"), depth, inp["x"])
    else:
        normals = d64("free_normals").requires_grad_(True)
    terms = geom_ref.geometry_terms(depth, inp["x"], d64("depth_gt"), normals, d64("normals_gt"), W, reg=True)
    total = sum(v[0] for v in terms.values())
    grads = torch.autograd.grad(total, [depth] if through_rays else [depth, normals])
    return terms, grads[0], (None if through_rays else grads[1])


# 1 patch: R = 64 < one workgroup; 5: R = 320, a partial last workgroup; 4099: R = 262336 rays, above the
# 1024 workgroups x 256 threads of the partial-sum grid (every thread strides)
@pytest.mark.parametrize("through_rays", [False, True], ids=["dn", "rays"])
@pytest.mark.parametrize("n_patches", [1, 5, 4099])
def test_kernel_shapes(dev, n_patches, through_rays):
    inp = node_inputs(n_patches)
    g = {k: (v.to(dev) if isinstance(v, torch.Tensor) else {q: t.to(dev) for q, t in v.items()}) for k, v in inp.items()}
    depth = g["depth"].clone().requires_grad_(True)
    if through_rays:
        normals = extract_normals_from_ray_batch(g["rays_o"], g["rays_d"], depth, g["x"])
        rays = (g["rays_o"], g["rays_d"])
    else:
        normals, rays = g["free_normals"].clone().requires_grad_(True), None
    vals, row, counts = geometry_losses(depth, g["x"], g["depth_gt"], normals, g["normals_gt"], ALL, W, step=7,
                                        reg_start=6, rays=rays)
    sum(vals).backward()
    torch.cuda.synchronize()
    terms, gd, gn = reference64(inp, through_rays)
    T = inp["x"]["x1"].numel()
    n_depth = int((inp["depth_gt"] > 0).sum())
    n_norm = int((inp["normals_gt"][inp["x"]["x1"]].abs().sum(-1) > 0).sum())
    assert counts.tolist() == [n_depth, n_norm, n_norm, T, 1, 1, 1, 1]
    assert torch.equal(row[:4], torch.stack(vals).detach())
    for i, k in enumerate(KEYS):
        loss64, scale, addends = terms[k]
        bound = fixed_order_bound(scale, addends)
        print(f"{k}: got {float(vals[i])!r} float64 {float(loss64)!r} |diff| {abs(float(vals[i]) - float(loss64)):.3e} "
              f"bound {bound:.3e}")
        assert abs(float(vals[i]) - float(loss64)) <= bound, k
        raw = float(addends.sum())
        assert abs(float(row[4 + i]) - raw) <= 2.0 ** -23 * abs(raw) + fixed_order_bound(1.0, addends)
    err = rel_l2(depth.grad, gd)
    print(f"d / d depth: rel. L2 {err:.3e}")
    assert err <= GRAD_BOUND
    if not through_rays:
        err = rel_l2(normals.grad, gn)
        print(f"d / d normals: rel. L2 {err:.3e}")
        assert err <= GRAD_BOUND


def test_one_valid_element(dev):
    """One depth label > 0 and one non-zero GT normal in a 64-ray patch.  A mean of one addend has the
    fixed-order bound 0, so addends and weights are chosen exact in float32: (2.5 - 2)^2, a predicted
    normal parallel to its label (cos = 1; L1 = |1 - 2|), weights that are powers of two."""
    inp = node_inputs(1)
    x = {k: v.to(dev) for k, v in inp["x"].items()}
    ray, tri = 37, 20
    depth = inp["depth"].clone()
    depth[ray] = 2.5
    depth_gt = torch.zeros(64)
    depth_gt[ray] = 2.0
    normals = inp["free_normals"].clone()
    normals[tri] = torch.tensor([0.0, 0.0, 1.0])
    normals_gt = torch.zeros(64, 3)
    normals_gt[int(inp["x"]["x1"][tri])] = torch.tensor([0.0, 0.0, 2.0])
    depth_g = depth.to(dev).requires_grad_(True)
    normals_g = normals.to(dev).requires_grad_(True)
    terms_bits = GEOM_DEPTH | GEOM_NORM_L1 | GEOM_NORM_DOT
    w = (0.125, 0.25, 0.5)
    vals, row, counts = geometry_losses(depth_g, x, depth_gt.to(dev), normals_g, normals_gt.to(dev), terms_bits, w)
    sum(vals).backward()
    torch.cuda.synchronize()
    assert counts.tolist() == [1, 1, 1, 0, 1, 1, 1, 0]
    d64 = depth.double().requires_grad_(True)
    n64 = normals.double().requires_grad_(True)
    ref = geom_ref.geometry_terms(d64, inp["x"], depth_gt.double(), n64, normals_gt.double(), w)
    gd, gn = torch.autograd.grad(sum(v[0] for v in ref.values()), [d64, n64])
    for i, k in enumerate(KEYS[:3]):
        loss64, scale, addends = ref[k]
        assert abs(float(vals[i]) - float(loss64)) <= fixed_order_bound(scale, addends), (k, float(vals[i]), float(loss64))
    assert float(vals[0]) == 0.125 * 0.25 and float(vals[1]) == 0.25 and float(vals[2]) == 0.0  # (cos = 1 exactly)
    assert float(vals[3]) == 0.0  # RegNeRF off
    assert rel_l2(depth_g.grad, gd) <= GRAD_BOUND and rel_l2(normals_g.grad, gn) <= GRAD_BOUND
    assert int((depth_g.grad != 0).sum()) == 1 and int((normals_g.grad != 0).any(-1).sum()) == 1


@pytest.mark.parametrize("through_rays", [False, True], ids=["dn", "rays"])
@pytest.mark.parametrize("what", ["empty", "nan", "inf", "not_started"])
def test_filtered_terms_give_exact_zeros(dev, what, through_rays):
    """An empty mask, a NaN and an Inf sum, a RegNeRF term before its start: the term is exactly 0 and
    its gradient exactly zero and finite, although the inputs of its backward hold the NaN."""
    inp = node_inputs(5)
    g = {k: v.to(dev) for k, v in inp.items() if isinstance(v, torch.Tensor)}
    x = {k: v.to(dev) for k, v in inp["x"].items()}
    depth, depth_gt, normals_gt = g["depth"].clone(), g["depth_gt"].clone(), g["normals_gt"].clone()
    step = 7
    if what == "empty":
        depth_gt.zero_()
        normals_gt.zero_()
        step = 6
    elif what == "not_started":
        step = 6
    else:  # in a ray that is the x1 corner of a triangle, with valid labels
        ray = int(inp["x"]["x1"][60])
        depth[ray] = float("nan") if what == "nan" else float("inf")
        depth_gt[ray] = 1.0
        normals_gt[ray] = torch.tensor([0.0, 1.0, 0.0], device=dev)
    depth.requires_grad_(True)
    if through_rays:
        normals = extract_normals_from_ray_batch(g["rays_o"], g["rays_d"], depth, x)
        rays = (g["rays_o"], g["rays_d"])
    else:
        normals, rays = g["free_normals"].clone().requires_grad_(True), None
        if what in ("nan", "inf"):
            with torch.no_grad():
                normals[60] = float("nan")
    vals, row, counts = geometry_losses(depth, x, depth_gt, normals, normals_gt, ALL, W, step=step, reg_start=6, rays=rays)
    sum(vals).backward()
    torch.cuda.synchronize()
    if what == "not_started":
        assert counts[4:].tolist() == [1, 1, 1, 0] and float(vals[3]) == 0.0 and all(float(v) > 0 for v in vals[:3])
        return
    assert counts[4:].tolist() == [0, 0, 0, 0]
    if what == "empty":
        assert counts[:4].tolist() == [0, 0, 0, 0]
    assert [float(v) for v in vals] == [0.0] * 4
    grads = [depth.grad] + ([] if through_rays else [normals.grad])
    for gr in grads:
        assert bool(torch.isfinite(gr).all()) and not bool(gr.any())


@pytest.mark.parametrize("n_patches", [5, 4099])
def test_two_runs_are_bit_identical(dev, n_patches):
    """The forward's row (every term, fixed-order sums) and the depth term's backward (one thread per
    ray, no atomics); the normal terms' dL/dnormals as well."""
    inp = node_inputs(n_patches)
    g = {k: v.to(dev) for k, v in inp.items() if isinstance(v, torch.Tensor)}
    x = {k: v.to(dev) for k, v in inp["x"].items()}
    rows, grads = [], []
    for _ in range(2):
        depth = g["depth"].clone().requires_grad_(True)
        normals = g["free_normals"].clone().requires_grad_(True)
        vals, row, counts = geometry_losses(depth, x, g["depth_gt"], normals, g["normals_gt"], ALL, W, step=7, reg_start=6)
        rows.append((row.clone(), counts.clone()))
        (vals[0] + vals[1] + vals[2]).backward()  # (without the RegNeRF scatter)
        grads.append((depth.grad.clone(), normals.grad.clone()))
    torch.cuda.synchronize()
    assert torch.equal(rows[0][0].view(torch.int32), rows[1][0].view(torch.int32)) and torch.equal(rows[0][1], rows[1][1])
    assert torch.equal(grads[0][0].view(torch.int32), grads[1][0].view(torch.int32))
    assert torch.equal(grads[0][1].view(torch.int32), grads[1][1].view(torch.int32))
    assert bool(grads[0][0].any()) and bool(grads[0][1].any())


def test_both_routes_of_the_normal_terms_agree(dev):
    """dL/dnormals handed on to _Normals.backward (pose refinement's route) against the normal terms
    carried to the depth inside the node: the same gradient up to float32 rounding of two orders."""
    inp = node_inputs(5)
    g = {k: v.to(dev) for k, v in inp.items() if isinstance(v, torch.Tensor)}
    x = {k: v.to(dev) for k, v in inp["x"].items()}
    out = []
    for rays in (None, (g["rays_o"], g["rays_d"])):
        depth = g["depth"].clone().requires_grad_(True)
        normals = extract_normals_from_ray_batch(g["rays_o"], g["rays_d"], depth, x)
        vals, _, _ = geometry_losses(depth, x, None, normals, g["normals_gt"], GEOM_NORM_L1 | GEOM_NORM_DOT, W, rays=rays)
        sum(vals).backward()
        out.append(depth.grad.clone())
    torch.cuda.synchronize()
    assert rel_l2(out[1], out[0].cpu()) <= 1e-5


def test_module_keeps_its_refusals(dev):
    """loss_norm_can_end with a device step is still host control flow; the normal terms need
    pred_norm_depth (the reference asserts it)."""
    h = dict(loss_depth_w=0.1, loss_reg_depth_w=1.0, loss_norm_can_end=4000, ray_sampling_strategy="all_images_triang")
    depth = torch.rand(192, device=dev)
    pred = dict(rgb=torch.rand(192, 3, device=dev), depth=depth, opacity=torch.zeros(192, device=dev),
                rays_o=torch.rand(192, 3, device=dev), rays_d=torch.rand(192, 3, device=dev))
    target = dict(rgb=torch.rand(192, 3, device=dev), depth=depth + 0.1, normals=torch.rand(192, 3, device=dev))
    with pytest.raises(NotImplementedError, match="loss_norm_can_end == -1"):
        NeRFMTLoss(h)(pred, target, global_step=torch.tensor(5, device=dev))
    ld = NeRFMTLoss(dict(h, loss_norm_can_end=-1))(pred, target, global_step=torch.tensor(5, device=dev))
    assert set(ld) == {"rgb", "depth", "reg_depth", "total"}
    with pytest.raises(ValueError, match="pred_norm_depth"):
        NeRFMTLoss(dict(h, loss_norm_depth_L1_w=0.1))(pred, target, global_step=5)
    assert losses.GEOM_KEYS == KEYS
