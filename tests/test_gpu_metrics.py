"""ncnerf_amd.metrics on the GPU against the host restatement (tests/metrics_ref.py).

The criterion, per pixel of a map and for each mean: |got - ref| <= 4 E + 2^-20, with ref the
float64 definition on the same float32 inputs and E the error that the float32 torch restatement in
the reference's dense structure makes against that same ref on that input (its per-pixel maximum for
maps, its mean's error for means).  4 allows another summation order; 2^-20 is 16 float32 ulps at 1.
E is computed on the CPU, from the restatement alone: the kernel never sets its own bound.
"""
import functools
import math

import numpy as np
import pytest
import torch

import metrics_ref as M

pytestmark = pytest.mark.gpu

from ncnerf_amd import _lib  # noqa: E402
from ncnerf_amd import metrics as NM  # noqa: E402  (fails on a tree without the feature)

BOUND0 = 2.0 ** -20


def _close(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


CASES = {"noise": M.noise_case, "flat": M.flat_case}


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@functools.lru_cache(maxsize=None)
def ssim_reference(case, h, w):
    """(pred, gt, [(map f64, mean)] x 3, [(E map, E mean)] x 3): computed once per case on the CPU."""
    pred, gt = CASES[case](h, w)
    ref = M.ssims_f64(pred, gt, h, w)
    t32 = M.ssims_torch32(pred, gt, h, w)
    E = [(float(np.abs(t32[k][0].double().numpy() - ref[k][0]).max()), abs(float(t32[k][1]) - ref[k][1]))
         for k in range(3)]
    return pred, gt, ref, E


# ---------------------------------------------------------------- SSIM
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("hw", [(11, 11), (12, 29), (37, 53), (70, 131), (96, 128)])
def test_ssim_maps_and_means(dev, case, hw):
    h, w = hw
    pred, gt, ref, E = ssim_reference(case, h, w)
    p, t = _dev(pred, dev), _dev(gt, dev)
    ssim, maps = NM.ssim_view(p, t, h, w, maps=True)
    ssim2, maps2 = NM.ssim_view(p, t, h, w, maps=True)
    assert torch.equal(ssim.view(torch.int32), ssim2.view(torch.int32)), "two calls differ"
    assert torch.equal(maps.view(torch.int32), maps2.view(torch.int32)), "two calls differ"
    ssim_no_maps, none = NM.ssim_view(p, t, h, w)
    assert none is None and torch.equal(ssim.view(torch.int32), ssim_no_maps.view(torch.int32))
    got_means, got_maps = ssim.cpu().double().numpy(), maps.cpu().double().numpy()
    for k, (name, rad) in enumerate((("ssim", 5), ("ssim_n", 5), ("ssim_n_sck", 3))):
        inside = got_maps[k][rad:h - rad, rad:w - rad]
        outside = got_maps[k].copy()
        outside[rad:h - rad, rad:w - rad] = np.nan
        assert np.isnan(outside).all(), f"{name}: a pixel whose window leaves the image was written"
        err_map = float(np.abs(inside - ref[k][0]).max())
        err_mean = abs(got_means[k] - ref[k][1])
        print(f"{case} {h}x{w} {name}: E map {E[k][0]:.2e} mean {E[k][1]:.2e}; kernel map {err_map:.2e} "
              f"mean {err_mean:.2e}")
        assert err_map <= 4 * E[k][0] + BOUND0, (name, err_map, E[k][0])
        assert err_mean <= 4 * E[k][1] + BOUND0, (name, err_mean, E[k][1])


def test_ssim_small_image_raises(dev):
    pred, gt = M.noise_case(10, 40)
    with pytest.raises(ValueError, match="11x11"):
        NM.ssim_view(_dev(pred, dev), _dev(gt, dev), 10, 40)
    with pytest.raises(ValueError, match="11x11"):
        NM.ViewMetrics().update({"rgb": _dev(pred, dev)}, {"rgb": _dev(gt, dev)}, 40, 10)
    ws = torch.empty(64, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.NcnError, match="11x11"):  # the library's own check
        _lib.call("ncn_metrics_ssim", _dev(pred, dev), _dev(gt, dev), 10, 40, torch.zeros(2, device=dev), ws, 64, None,
                  torch.zeros(3, device=dev))


# ---------------------------------------------------------------- selection
def _values(kind, n, rng):
    if kind == "equal":
        return np.full(n, 37.25, np.float32)
    if kind == "ties":
        return rng.integers(0, 5, n).astype(np.float32) * np.float32(22.5)
    if kind == "ends":  # 0.0 and 180.0 among angles, denormal-small and ordinary ones
        v = (rng.random(n, dtype=np.float32) * np.float32(180.0)).astype(np.float32)
        v[rng.integers(0, n, max(n // 3, 1))] = 0.0
        v[rng.integers(0, n, max(n // 3, 1))] = 180.0
        v[rng.integers(0, n, max(n // 8, 1))] = 1e-40
        return v
    return (rng.random(n, dtype=np.float32) ** 3 * np.float32(180.0)).astype(np.float32)  # "marked"


@pytest.mark.parametrize("kind", ["equal", "ties", "ends", "marked"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097, 9170])
def test_select_median_is_kthvalue_bit_for_bit(dev, n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    vals = _values(kind, n, rng)
    k = (n - 1) // 2
    want = torch.kthvalue(torch.from_numpy(vals), k + 1).values
    arr = vals
    if kind == "marked":  # invalid entries interleaved: two of three slots carry the marker
        arr = np.full(3 * n + 5, np.nan, np.float32)
        arr.view(np.uint32)[:] = M.MARK
        arr[rng.permutation(3 * n + 5)[:n]] = vals
    both = np.stack([arr, arr[::-1]])  # two rows at once, the second reversed
    n_dev = torch.tensor([n], dtype=torch.int64, device=dev)  # n is read on the device
    got = NM.select_median(_dev(both, dev), n_dev)
    got2 = NM.select_median(_dev(arr, dev), n_dev)
    assert got.shape == (2,) and got2.shape == (1,)
    bits = got.cpu().view(torch.int32).tolist() + got2.cpu().view(torch.int32).tolist()
    assert bits == [want.view(torch.int32).item()] * 3, (got.tolist(), want.item())


def test_select_median_wrong_n_is_nan(dev):
    arr = _dev(np.arange(10, dtype=np.float32), dev)
    for n in (0, 11, -3):
        assert math.isnan(NM.select_median(arr, torch.tensor([n], dtype=torch.int64, device=dev)).item())
    marked = np.arange(10, dtype=np.float32)
    marked.view(np.uint32)[:] = M.MARK  # a rank past the unmarked entries
    assert math.isnan(NM.select_median(_dev(marked, dev), torch.tensor([3], dtype=torch.int64, device=dev)).item())


# ---------------------------------------------------------------- angles
AH, AW = 70, 131


@functools.lru_cache(maxsize=None)
def angle_case():
    rng = np.random.default_rng(5)
    n = AH * AW
    pred = rng.standard_normal((n, 3)).astype(np.float32)
    gt = rng.standard_normal((n, 3)).astype(np.float32)
    gt[rng.permutation(n)[:n // 3]] = 0.0  # a third of the ground truth is invalid
    pred[rng.permutation(n)[:50]] = 0.0    # zero predictions: 90 degrees
    valid, a, m = M.angles_f64(pred, gt)
    a32, m32 = M.angles_torch32(pred, gt)
    E = max(float(np.abs(a32.double().numpy() - a).max()), float(np.abs(m32.double().numpy() - m).max()))
    means32 = M.normals_torch32(pred, gt)
    E_mean = (abs(float(means32[0]) - a.mean()), abs(float(means32[2]) - m.mean()))
    return pred, gt, valid, a, m, E, E_mean


def _angles(pred, gt, dev):
    n = pred.shape[0]
    angles = torch.empty(2, n, dtype=torch.float32, device=dev)
    ws = torch.empty(4 * min(-(-n // 256), 1024), dtype=torch.float64, device=dev)
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.call("ncn_metrics_angles", _dev(pred, dev), _dev(gt, dev), n, angles, ws, ws.numel(), sums, counts)
    return angles, sums, counts


def _normal_row(pred, gt, h, w, dev):
    rgb = torch.rand(h * w, 3, device=dev)
    vm = NM.ViewMetrics(norm_gt=True)
    vm.update({"rgb": rgb, "norm_depth": _dev(pred, dev)}, {"rgb": rgb + 0.1, "normals": _dev(gt, dev)}, h, w)
    return vm


def test_angles_per_pixel_means_and_medians(dev):
    """The means are held to 4 E at the kernel's float64 sums / n; the row's float32 value must be
    exactly that quotient rounded (a float32 near 90 cannot be closer than 3.8e-6 to anything)."""
    pred, gt, valid, a, m, E, E_mean = angle_case()
    angles, sums, counts = _angles(pred, gt, dev)
    angles2, sums2, _ = _angles(pred, gt, dev)
    assert torch.equal(angles.view(torch.int32), angles2.view(torch.int32)) and torch.equal(sums, sums2)
    n_valid = int(valid.sum())
    assert counts.tolist() == [n_valid, 0]
    got = angles.cpu()
    marked = got.view(torch.int32).numpy() == -1
    assert np.array_equal(marked[0], ~valid) and np.array_equal(marked[1], ~valid)
    ga, gm = got[0].double().numpy()[valid], got[1].double().numpy()[valid]
    err = max(float(np.abs(ga - a).max()), float(np.abs(gm - m).max()))
    bound = 4 * E + BOUND0
    print(f"angles {AH}x{AW}: {n_valid} valid; E per pixel {E:.2e}, kernel {err:.2e}; E of the means {E_mean}")
    assert err <= bound, (err, E)
    zero_pred = (np.abs(pred).sum(-1) == 0)[valid]
    assert zero_pred.sum() >= 20 and np.all(ga[zero_pred] == 90.0) and np.all(gm[zero_pred] == 90.0)
    mean_dev = (sums.cpu().numpy() / n_valid).tolist()
    for got_mean, ref_mean, e in zip(mean_dev, (a.mean(), m.mean()), E_mean):
        print(f"  mean: kernel {abs(got_mean - ref_mean):.2e}, E {e:.2e}")
        assert abs(got_mean - ref_mean) <= 4 * e + BOUND0
    row = _normal_row(pred, gt, AH, AW, dev).rows()[0].cpu()
    assert row[11] == 1.0
    assert row[7].item() == np.float32(mean_dev[0]) and row[9].item() == np.float32(mean_dev[1])
    # the medians: exactly torch.kthvalue of the kernel's own angles, and within the per-pixel bound
    # of the definition's medians (the median is 1-Lipschitz in the sup norm)
    k = (n_valid - 1) // 2 + 1
    for col, r, ref_vals in ((8, 0, a), (10, 1, m)):
        assert row[col].item() == torch.kthvalue(got[r][torch.from_numpy(valid)], k).values.item()
        assert abs(row[col].item() - M.median_lower(ref_vals)) <= bound


def test_angles_nan_and_not_counted(dev):
    pred, gt, valid, *_ = angle_case()
    bad = pred.copy()
    bad[np.nonzero(valid)[0][7], 1] = np.nan
    vm = _normal_row(bad, gt, AH, AW, dev)
    row = vm.rows()[0].tolist()
    assert all(math.isnan(v) for v in row[7:11]) and row[11] == 1.0
    assert all(math.isnan(vm.compute()[f"norm_depth/ang_err_{k}"]) for k in ("mean", "median", "mean_min", "median_min"))
    bad = pred.copy()
    bad[np.nonzero(~valid)[0][3], 2] = np.nan  # on an invalid pixel: nothing changes
    assert torch.equal(_normal_row(bad, gt, AH, AW, dev).rows()[:, 7:], _normal_row(pred, gt, AH, AW, dev).rows()[:, 7:])
    # a view with no valid ground truth is not counted and is left out of compute()
    vm = _normal_row(pred, gt, AH, AW, dev)
    first = vm.rows()[0].tolist()
    rgb = torch.rand(AH * AW, 3, device=dev)
    vm.update({"rgb": rgb, "norm_depth": _dev(pred, dev)}, {"rgb": rgb + 0.1, "normals": _dev(np.zeros_like(gt), dev)},
              AH, AW)
    rows = vm.rows().tolist()
    assert rows[1][7:] == [0.0] * 5 and rows[0] == first
    logs = vm.compute()
    assert logs["norm_depth/ang_err_mean"] == first[7] and logs["norm_depth/ang_err_median_min"] == first[10]
    alone = NM.ViewMetrics(norm_gt=True)
    alone.update({"rgb": rgb, "norm_depth": _dev(pred, dev)}, {"rgb": rgb + 0.1, "normals": _dev(np.zeros_like(gt), dev)},
                 AH, AW)
    assert math.isnan(alone.compute()["norm_depth/ang_err_median"])  # 0 / 0, as in the reference


# ---------------------------------------------------------------- depth and the rgb error
@pytest.mark.parametrize("n", [1, 65, 9170])
def test_pointwise_sums(dev, n):
    """Fixed-order sums against the exact sum of the same float32 terms: 2 (n - 1) 2^-24 sum|terms|."""
    rng = np.random.default_rng(n)
    gt = (rng.random(n, dtype=np.float32) * 5 + np.float32(0.5)).astype(np.float32)
    pred = (gt + rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    if n > 1:
        gt[1::7] = 0.0
        gt[2::11] = -1.5
        gt[3] = np.nan
    rgb_t = rng.random((n, 3), dtype=np.float32)
    rgb_p = (rgb_t + np.float32(0.05) * rng.standard_normal((n, 3)).astype(np.float32)).astype(np.float32)
    ws = torch.empty(6 * min(-(-n // 256), 1024), dtype=torch.float64, device=dev)
    sums = torch.empty(3, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    rng_out = torch.empty(2, dtype=torch.float32, device=dev)
    args = (_dev(rgb_p, dev), _dev(rgb_t, dev), _dev(pred, dev), _dev(gt, dev), n, ws, ws.numel())
    _lib.call("ncn_metrics_pointwise", *args, sums, count, rng_out)
    sums2 = torch.empty_like(sums)
    _lib.call("ncn_metrics_pointwise", *args, sums2, count, rng_out)
    assert torch.equal(sums, sums2)
    with np.errstate(invalid="ignore"):
        valid = gt > 0
    d = (pred[valid] - gt[valid]).astype(np.float32)
    drgb = (rgb_p - rgb_t).astype(np.float32).reshape(-1)
    terms = [(drgb * drgb).astype(np.float32), (d * d).astype(np.float32), np.abs(d)]
    got = sums.tolist()
    assert count.item() == int(valid.sum())
    assert rng_out.tolist() == [float(rgb_t.min()), float(rgb_t.max())]
    for g, t in zip(got, terms):
        ref = float(t.astype(np.float64).sum())
        bound = 2 * (t.size - 1) * 2.0 ** -24 * float(np.abs(t).astype(np.float64).sum())
        print(f"n={n}: |sum - ref| = {abs(g - ref):.3e}, bound {bound:.3e}")
        assert abs(g - ref) <= bound


def test_depth_columns_and_all_invalid_view(dev):
    h, w = 11, 13
    n = h * w
    rng = np.random.default_rng(2)
    rgb = torch.rand(n, 3, device=dev)
    gt = (rng.random(n, dtype=np.float32) * 3).astype(np.float32)
    gt[::5], gt[1::9], gt[7] = 0.0, -2.0, np.nan
    pred = (np.nan_to_num(gt) + rng.standard_normal(n).astype(np.float32) * np.float32(0.1)).astype(np.float32)
    vm = NM.ViewMetrics(eval_depth=True)
    vm.update({"rgb": rgb, "depth": _dev(pred, dev)}, {"rgb": rgb + 0.1, "depth": _dev(gt, dev)}, h, w)
    dead = np.where(np.arange(n) % 2 == 0, 0.0, -1.0).astype(np.float32)
    dead[5] = np.nan
    vm.update({"rgb": rgb, "depth": _dev(pred, dev)}, {"rgb": rgb + 0.1, "depth": _dev(dead, dev)}, h, w)
    rows = vm.rows().tolist()
    rmse, ab, counted = M.depth_f64(pred, gt)
    assert counted == 1 and rows[0][6] == 1.0
    assert abs(rows[0][4] - rmse) <= 1e-6 * rmse and abs(rows[0][5] - ab) <= 1e-6 * ab
    assert rows[1][4:7] == [0.0, 0.0, 0.0]  # not counted
    assert all(abs(r[0] - 20.0) <= 1e-4 for r in rows)
    logs = vm.compute()
    assert logs["depth/rmse"] == rows[0][4] and logs["depth/abs"] == rows[0][5]
    assert set(logs) == {"rgb/psnr", "rbg/ssim", "rbg/ssim_n", "rbg/ssim_n_sck", "depth/rmse", "depth/abs"}


# ---------------------------------------------------------------- ViewMetrics and evaluate_views
def test_view_metrics_through_evaluate_views(dev, monkeypatch):
    """The 96x128, V = 2 scene of test_gpu_eval.test_evaluate_views with ground truths made from the
    renders plus offsets: rows against the float64 restatement, compute() against the restatement's
    averaging of rows(), and ONE device-to-host copy outside the renderer and the clustering."""
    import ncnerf_amd.evaluation as Ev
    import ncnerf_amd.rendering as rendering
    from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
    from ncnerf_amd.synthetic import SyntheticScene
    from test_gpu_eval import dir_grid
    scene = SyntheticScene()
    torch.manual_seed(0)
    model = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with torch.no_grad():
        model.density_grid.copy_(torch.from_numpy(scene.density_grid).to(dev) * 10.0)
        model.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    H, W, V = 96, 128, 2
    dirs = _dev(dir_grid(H, W), dev)
    poses = _dev(scene.poses[:V], dev)
    rgbs, depths, norms = [], [], []
    with torch.no_grad():
        for v in range(V):
            rd = (dirs @ poses[v, :, :3].T).contiguous()
            ro = poses[v, :, 3].expand_as(rd).contiguous()
            res = rendering.render(model, ro, rd, near_distance=0.01, max_samples=1024, test_time=True)
            rgbs.append(res["rgb"].reshape(-1, 3).float())
            depths.append(res["depth"].reshape(-1).float())
            norms.append(Ev.extract_normals_from_depth_batch(res["depth"].reshape(1, H, W), dirs, poses[v:v + 1, :, :3])[0]
                         .reshape(-1, 3))
    torch.manual_seed(1)
    rgb_gt = torch.stack(rgbs) + 0.1
    depth_gt = torch.stack(depths) + 0.25
    depth_gt[1] = 0.0  # the second view has no valid depth: not counted
    normals_gt = torch.stack(norms) + 0.05 * torch.randn(V, H * W, 3, device=dev)
    normals_gt[:, ::3] = 0.0

    copies, watching, renders = [], [True], [0]
    for name in ("cpu", "numpy", "tolist", "item", "__float__", "__int__", "__bool__", "__index__"):
        orig = getattr(torch.Tensor, name)

        def spy(self, *a, _orig=orig, **k):
            if watching[0] and self.is_cuda:
                copies.append(self.numel())
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)
    orig_nc, orig_render = Ev.normals_clustering, rendering.render

    def nc_spy(*a, **k):
        watching[0] = False
        return orig_nc(*a, **k)

    def render_spy(*a, **k):
        watching[0] = False
        try:
            return orig_render(*a, **k)
        finally:
            watching[0] = True
            renders[0] += 1
    monkeypatch.setattr(Ev, "normals_clustering", nc_spy)
    monkeypatch.setattr(rendering, "render", render_spy)
    out = Ev.evaluate_views(model, poses, dirs, (W, H), rgb_gt=rgb_gt, K=30, niter=30, t_similar=0.99,
                            R_ref=torch.eye(3), depth_gt=depth_gt, normals_gt=normals_gt)
    monkeypatch.undo()
    assert renders[0] == V and not watching[0]
    assert copies == [V * 12], copies  # one copy: the V rows, after the last view

    old_keys = {"psnr", "psnr_mean", "normals", "labels", "centroids", "frame", "angles"}
    assert set(out) == old_keys | {"metrics", "per_view"}
    assert len(out["per_view"]) == V and all(tuple(r) == NM.COLUMNS for r in out["per_view"])
    assert out["psnr"] == [r["psnr"] for r in out["per_view"]] and all(abs(p - 20.0) <= 1e-3 for p in out["psnr"])
    rows = [[r[c] for c in NM.COLUMNS] for r in out["per_view"]]
    want_logs = M.compute_from_rows(rows, True, True)
    assert set(out["metrics"]) == set(want_logs)
    for key, val in want_logs.items():
        assert _close(out["metrics"][key], val, 1e-9 * max(1.0, abs(val))), key
    # the rows themselves against the float64 definitions on the same images
    tol = [1e-4, 1e-5, 1e-5, 1e-5, 1e-5, 1e-5, 0, 1e-3, 0.05, 1e-3, 0.05, 0]
    for v in range(V):
        preds = {"rgb": rgbs[v].cpu().numpy(), "depth": depths[v].cpu().numpy(), "norm_depth": norms[v].cpu().numpy()}
        target = {"rgb": rgb_gt[v].cpu().numpy(), "depth": depth_gt[v].cpu().numpy(),
                  "normals": normals_gt[v].cpu().numpy()}
        ref = M.view_row_f64(preds, target, H, W, True, True)
        print(f"view {v}: kernel {np.round(rows[v], 6).tolist()}\n        f64    {np.round(ref, 6).tolist()}")
        assert ref[6] == (1 if v == 0 else 0) and ref[11] == 1
        for c, name in enumerate(NM.COLUMNS):
            assert _close(rows[v][c], ref[c], tol[c]), (v, name, rows[v][c], ref[c])
    # ViewMetrics on its own, on this test's renders of the same views; no new argument, the old result
    vm = NM.ViewMetrics(eval_depth=True, norm_gt=True)
    for v in range(V):
        vm.update({"rgb": rgbs[v], "depth": depths[v], "norm_depth": norms[v]},
                  {"rgb": rgb_gt[v], "depth": depth_gt[v], "normals": normals_gt[v]}, H, W)
    assert vm.rows().shape == (V, 12) and vm.rows().is_cuda
    for mine, theirs in zip(vm.rows().tolist(), rows):
        assert all(_close(a, b, t) for a, b, t in zip(mine, theirs, tol)), (mine, theirs)
    own = vm.compute()
    want = M.compute_from_rows(vm.rows().tolist(), True, True)
    assert set(own) == set(want) and all(_close(own[k], want[k], 1e-9 * max(1.0, abs(want[k]))) for k in want)
    plain = Ev.evaluate_views(model, poses, dirs, (W, H), rgb_gt=rgb_gt, K=30, niter=30, t_similar=0.99,
                              R_ref=torch.eye(3))
    assert set(plain) == old_keys
    assert all(abs(a - b) <= 1e-4 for a, b in zip(plain["psnr"], out["psnr"]))
    only = Ev.evaluate_views(model, poses, dirs, (W, H), rgb_gt=rgb_gt, K=30, niter=30, R_ref=torch.eye(3), metrics=True)
    assert set(only["metrics"]) == {"rgb/psnr", "rbg/ssim", "rbg/ssim_n", "rbg/ssim_n_sck"}
    with pytest.raises(ValueError, match="rgb_gt"):
        Ev.evaluate_views(model, poses, dirs, (W, H), metrics=True)
