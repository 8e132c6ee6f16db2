"""The Manhattan-frame evaluation on the device (ncnerf_amd.evaluation: ncn_depth_normals_image,
ncn_kmeans_train, ncn_kmeans_assign) against the reference's image normals (tests/golden/
depth_normals_image.npz), a float64 evaluation of the same formula, and the oracle's restatement
of faiss's spherical k-means (oracle/losses_ref.py), which the kernels follow operation for
operation.

Tolerances
  image normals   per component <= (4 |a||b| / |a x b| + 8) 2^-24 against float64 from the same f32
                  points (a, b the two edge vectors: one rounding per product of the cross product,
                  carried through normalisation and rotation); pixels with |a x b| < 2^-20 |a||b|
                  are left out, at most 1 % of them.  The same bound holds against the reference's
                  own output (the fixture).
  k-means         assignments and counts equal, centroids atol 1e-5 (test_gpu_loss.py's bound for
                  the training step's kernel), two runs bit-identical.
  frame           centrs_new of the HIP pipeline within 1e-5 of the CPU pipeline's (numpy image
                  normals + oracle k-means + selection); column angles to the known rotation at
                  most 0.1 degree above the CPU pipeline's.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import losses_ref
from ncnerf_amd import _lib
from ncnerf_amd import evaluation as E
from ncnerf_amd.synthetic import SCENE_MAX, SCENE_MIN, make_cameras

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24


# ---------------------------------------------------------------- helpers (host, no GPU)
def dir_grid(H, W, hfov=math.radians(70.0)):
    fx = (W / 2) / math.tan(hfov / 2)
    u, v = np.meshgrid(np.arange(W, dtype=np.float32) + 0.5, np.arange(H, dtype=np.float32) + 0.5)
    d = np.stack([(u - W / 2) / fx, (v - H / 2) / fx, np.ones_like(u)], -1).reshape(-1, 3)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def box_room_depth(c2w, dirs, H, W, noise, seed):
    """Distance to the walls of the scene box from inside, per view (B,H,W), with multiplicative noise."""
    rng = np.random.default_rng(seed)
    out = np.empty((len(c2w), H, W), np.float32)
    for b, P in enumerate(c2w):
        d = (dirs @ P[:, :3].T).astype(np.float32)
        o = P[:, 3][None]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(d > 0, (SCENE_MAX[None] - o) / d, (SCENE_MIN[None] - o) / d)
        t = np.where(np.isfinite(t) & (t > 0), t, np.inf).min(axis=1).astype(np.float32)
        out[b] = (t * (1 + noise * rng.standard_normal(H * W)).astype(np.float32)).reshape(H, W)
    return out


def normals_image_np(depth, dirs, rot, dtype):
    """The formula of ncn_depth_normals_image from the f32 points P = dirs * depth, evaluated in
    `dtype` (float32: the kernel's operations in its order; float64: the yardstick).
    -> (normals (B,H,W,3), |a|, |b|, |a x b| on the interior in float64)."""
    B, H, W = depth.shape
    with np.errstate(invalid="ignore", over="ignore"):
        P = (dirs.reshape(1, H, W, 3) * depth[..., None]).astype(np.float32).astype(dtype)
        P1, P2, P3 = P[:, 1:-1, 1:-1], P[:, :-2, 1:-1], P[:, 1:-1, :-2]
        a, b = P2 - P1, P3 - P1
        c = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
        nrm = np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])
        n = c / np.maximum(nrm, dtype(1e-12))[..., None]
        R = rot.astype(dtype)[:, None, None]  # (B,1,1,3,3)
        n = (R[..., 0] * n[..., None, 0] + R[..., 1] * n[..., None, 1]) + R[..., 2] * n[..., None, 2]
        out = np.zeros((B, H, W, 3), dtype)
        out[:, 1:-1, 1:-1] = n
        d = depth
        out[(d == 0) | np.isnan(d) | np.isinf(d)] = 0
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        return (out, np.linalg.norm(a64, axis=-1), np.linalg.norm(b64, axis=-1),
                np.linalg.norm(np.cross(a64, b64), axis=-1))


def check_normals_bound(got, depth, dirs, rot, ref=None):
    """got (B,H,W,3) against float64 (or `ref`) under the module doc's bound on the
    interior pixels that are finite in float64; returns the worst error / bound."""
    n64, la, lb, lc = normals_image_np(depth, dirs, rot, np.float64)
    ref = n64 if ref is None else ref
    fin = np.isfinite(n64[:, 1:-1, 1:-1]).all(-1) & np.isfinite(lc) & (la * lb > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        keep = fin & (lc >= 2.0 ** -20 * la * lb)
        bound = (4 * la * lb / lc + 8) * U
    own_ok = ~((depth == 0) | np.isnan(depth) | np.isinf(depth))[:, 1:-1, 1:-1]
    keep &= own_ok
    left_out = int((fin & own_ok & ~keep).sum())
    assert left_out <= 0.01 * fin.size, left_out
    err = np.abs(got[:, 1:-1, 1:-1].astype(np.float64) - ref[:, 1:-1, 1:-1].astype(np.float64)).max(-1)
    ratio = float((err[keep] / bound[keep]).max())
    print(f"image normals: worst error / bound = {ratio:.3f} over {int(keep.sum())} pixels (left out {left_out})")
    assert ratio <= 1.0, ratio
    return ratio


def rotated_manhattan_normals(n, seed, noise=0.03, outliers=0.1):
    """Noisy normals of a rotated Manhattan room + `outliers` uniformly random directions, unit f32."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    R = Rotation.random(random_state=seed).as_matrix()
    axes = np.concatenate([R.T, -R.T]).astype(np.float32)
    p = np.array([0.3, 0.25, 0.25, 0.05, 0.1, 0.05])
    x = axes[rng.choice(6, n, p=p)] + rng.normal(0, noise, (n, 3)).astype(np.float32)
    out = rng.random(n) < outliers
    x[out] = rng.normal(size=(int(out.sum()), 3)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, np.float32)


def degenerate_normals(n, seed):
    """Six exact directions: the 30 init picks repeat points, so 24 clusters are empty every round
    and faiss's split_clusters path runs."""
    rng = np.random.default_rng(seed)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    return np.ascontiguousarray(axes[rng.choice(6, n)])


@functools.lru_cache(maxsize=None)
def kmeans_case(kind, n, K, niter):
    """(X, oracle centroids, oracle assignments) — computed once per case, read-only."""
    X = degenerate_normals(n, seed=5) if kind == "degenerate" else rotated_manhattan_normals(n, seed=n)
    C, a = losses_ref.spherical_kmeans(X, K=K, niter=niter, seed=1234)
    for arr in (X, C, a):
        arr.setflags(write=False)
    return X, C, a


FRAME_H, FRAME_W = 48, 64


@functools.lru_cache(maxsize=None)
def frame_case():
    """Four 48x64 views of the box room (0.2 % depth noise), the world rotated by a known R."""
    from scipy.spatial.transform import Rotation
    R = Rotation.from_euler("ZYX", [25.0, -10.0, 5.0], degrees=True).as_matrix()
    c2w = make_cameras(8, seed=3)[:4]
    dirs = dir_grid(FRAME_H, FRAME_W)
    depth = box_room_depth(c2w, dirs, FRAME_H, FRAME_W, 0.002, seed=41)
    poses = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))
    poses[:, :3, :3] = (R[None] @ c2w[:, :, :3].astype(np.float64)).astype(np.float32)
    poses[:, :3, 3] = (c2w[:, :, 3].astype(np.float64) @ R.T).astype(np.float32)
    return R, depth, dirs, poses


@functools.lru_cache(maxsize=None)
def frame_cpu_pipeline():
    """numpy image normals (f32, the kernel's operations) -> validity filter -> oracle k-means
    (K=30, niter=30) -> selection -> (centrs_new, frame, column angles to R)."""
    R, depth, dirs, poses = frame_case()
    n32 = normals_image_np(depth, dirs, poses[:, :3, :3], np.float32)[0].reshape(-1, 3)
    X = n32[losses_ref.valid_normals_mask(torch.from_numpy(n32)).numpy()]
    C, a = losses_ref.spherical_kmeans(X, K=30, niter=30, seed=1234)
    _, cn = losses_ref.cluster_select(C, a, 0.99)
    F, ang = E.manhattan_frame(cn, R_ref=R)
    return cn, F, ang


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # (a copy: the cached cases are read-only)


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


# ---------------------------------------------------------------- image normals
def test_image_normals_fixture(dev):
    g = np.load(os.path.join(GOLD, "depth_normals_image.npz"))
    depth, dirs, poses, ref = g["depth"], g["dirs"], g["poses"], g["normals"]
    B, H, W = depth.shape
    out = E.extract_normals_from_depth_batch(_dev(depth, dev), _dev(dirs, dev), _dev(poses, dev))
    assert out.shape == (B, H, W, 3) and out.dtype == torch.float32
    got = out.cpu().numpy()
    rot = poses[:, :3, :3]
    check_normals_bound(got, depth, dirs, rot)                      # against float64
    check_normals_bound(got, depth, dirs, rot, ref=ref)             # against the reference's own output
    # the border is exactly zero
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert np.all(got[:, border] == 0.0)
    # zero / NaN / Inf depth pixels are exactly zero; NaN exactly where the reference has it
    bad = (depth == 0) | np.isnan(depth) | np.isinf(depth)
    assert int(bad.sum()) == 3 and np.all(got[bad] == 0.0)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    for (y, x) in zip(*np.nonzero(~np.isfinite(depth[0]))):  # right and lower neighbours of NaN / Inf depth
        assert np.isnan(got[0, y, x + 1]).all() and np.isnan(got[0, y + 1, x]).all()
    (zy,), (zx,) = np.nonzero(depth[0] == 0)
    assert np.isfinite(got[0, zy, zx + 1]).all() and np.isfinite(got[0, zy + 1, zx]).all()
    # (B,3,4) and (B,3,3) poses, and B = 1, give the same bits
    for p in (poses[:, :3], poses[:, :3, :3]):
        assert _same_bits(E.extract_normals_from_depth_batch(_dev(depth, dev), _dev(dirs, dev), _dev(p, dev)), out)
    one = E.extract_normals_from_depth_batch(_dev(depth[1:], dev), _dev(dirs, dev), _dev(poses[1:, :3], dev))
    assert one.shape == (1, H, W, 3) and _same_bits(one[0], out[1])


@pytest.mark.parametrize("H,W", [(3, 3), (3, 7), (9, 3), (2, 5)])
def test_image_normals_small_shapes(dev, H, W):
    """H = 3 / W = 3: a single interior row / column (3x3: one pixel); H = 2: no interior at all."""
    rng = np.random.default_rng(H * 16 + W)
    dirs = dir_grid(H, W)
    depth = rng.uniform(0.5, 2.0, (2, H, W)).astype(np.float32)
    rot = make_cameras(2, seed=1)[:, :, :3]
    out = torch.full((2, H, W, 3), 7.0, device=dev)  # every element is written
    dd, qd, rd = _dev(depth, dev), _dev(dirs, dev), _dev(rot, dev)
    _lib.call("ncn_depth_normals_image", dd, qd, rd, 2, H, W, out)
    got = out.cpu().numpy()
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert np.all(got[:, border] == 0.0)
    if H >= 3:
        assert np.all(np.abs(np.linalg.norm(got[:, 1:-1, 1:-1], axis=-1) - 1) < 1e-5)
        check_normals_bound(got, depth, dirs, rot)


def test_image_normals_frame_views(dev):
    R, depth, dirs, poses = frame_case()
    got = E.extract_normals_from_depth_batch(_dev(depth, dev), _dev(dirs, dev), _dev(poses, dev)).cpu().numpy()
    check_normals_bound(got, depth, dirs, poses[:, :3, :3])


# ---------------------------------------------------------------- k-means
KMEANS_CASES = [("manhattan", n, 30, 30) for n in (30, 31, 2000, 7680, 7681, 12548)] + [
    ("degenerate", 8000, 30, 30), ("degenerate", 600, 30, 30), ("manhattan", 2561, 10, 10)]


@pytest.mark.parametrize("kind,n,K,niter", KMEANS_CASES)
def test_kmeans_parity(dev, kind, n, K, niter):
    X, C, a = kmeans_case(kind, n, K, niter)
    Xd = _dev(X, dev)
    cents, assign, counts = E.spherical_kmeans(Xd, K, niter, seed=1234)
    cents2, assign2, counts2 = E.spherical_kmeans(Xd, K, niter, seed=1234)
    torch.cuda.synchronize()
    got_c, got_a, got_n = cents.cpu().numpy(), assign.cpu().numpy(), counts.cpu().numpy()
    print(f"k-means {kind} n={n} K={K}: max |dC| = {np.abs(got_c - C).max():.3e}, "
          f"assignments differing = {int((got_a != a).sum())}")
    assert assign.dtype == torch.int32 and counts.dtype == torch.int64
    assert np.array_equal(got_a, a)
    assert np.array_equal(got_n, np.bincount(a, minlength=K))
    np.testing.assert_allclose(got_c, C, atol=1e-5, rtol=0)
    assert _same_bits(cents, cents2)
    assert torch.equal(assign, assign2) and torch.equal(counts, counts2)


def test_assign_at_scale(dev):
    """n = 200 003: many workgroups of the stream, a tail that is no multiple of 64 or 256."""
    n, K = 200_003, 30
    X = rotated_manhattan_normals(n, seed=77)
    C = kmeans_case("manhattan", 2000, 30, 30)[1]
    ref = np.argmax(losses_ref._dots(X, C), axis=1)
    Xd, Cd = _dev(X, dev), _dev(C, dev)
    assign = torch.full((n + 64,), -5, dtype=torch.int32, device=dev)
    counts = torch.full((K + 2,), -5, dtype=torch.int64, device=dev)
    _lib.call("ncn_kmeans_assign", Xd, n, Cd, K, assign, counts)
    got, cnt = assign.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(got[:n], ref)
    assert np.all(got[n:] == -5) and np.all(cnt[K:] == -5)  # nothing written past the ends
    assert np.array_equal(cnt[:K], np.bincount(ref, minlength=K)) and int(cnt[:K].sum()) == n


def test_clustering_drops_invalid_rows(dev):
    """37 all-zero rows and one NaN row among the 2000 normals: exactly those are dropped, and the
    rest cluster as the 2000 alone."""
    X, C, a = kmeans_case("manhattan", 2000, 30, 30)
    rng = np.random.default_rng(3)
    pos = np.sort(rng.choice(2038, 38, replace=False))
    full = np.zeros((2038, 3), np.float32)
    keep = np.ones(2038, bool)
    keep[pos] = False
    full[keep] = X
    full[pos[5], 1] = np.nan
    new, ass, cn = E.normals_clustering(_dev(full, dev), K=30, niter=30, t_similar=0.99, merge_clusters=True,
                                        find_opposite=True)
    assert new.shape == (2000,) and ass.shape == (2000,) and cn.shape == (3, 3)
    assert new.dtype == torch.int64 and ass.dtype == torch.int64 and new.is_cuda and cn.is_cuda
    assert np.array_equal(ass.cpu().numpy(), a)
    lab, cn_ref = losses_ref.cluster_select(C, a, 0.99)
    assert np.array_equal(new.cpu().numpy(), lab)
    np.testing.assert_allclose(cn.cpu().numpy(), cn_ref, atol=1e-5, rtol=0)
    with pytest.raises(ValueError):
        E.normals_clustering(_dev(full[:60] * 0, dev), K=30)  # 60 rows, none valid
    with pytest.raises(ValueError):
        E.normals_clustering(_dev(X[:29], dev), K=30)  # N < K
    with pytest.raises(RuntimeError):
        E.normals_clustering(torch.from_numpy(np.array(X)), K=30)  # a host tensor, N >= K


# ---------------------------------------------------------------- frame
def test_frame_of_rotated_box_room(dev):
    R, depth, dirs, poses = frame_case()
    cn_cpu, F_cpu, ang_cpu = frame_cpu_pipeline()
    normals = E.extract_normals_from_depth_batch(_dev(depth, dev), _dev(dirs, dev), _dev(poses, dev))
    new, ass, cn = E.normals_clustering(normals, K=30, niter=30, t_similar=0.99, merge_clusters=True,
                                        find_opposite=False)
    F, ang = E.manhattan_frame(cn, R_ref=R)
    print(f"frame: column angles HIP {np.round(ang, 4).tolist()} deg, CPU pipeline {np.round(ang_cpu, 4).tolist()} deg, "
          f"max |d centrs_new| = {np.abs(cn.cpu().numpy() - cn_cpu).max():.3e}")
    assert new.shape[0] == 4 * (FRAME_H - 2) * (FRAME_W - 2)
    np.testing.assert_allclose(cn.cpu().numpy(), cn_cpu, atol=1e-5, rtol=0)
    assert np.all(ang <= ang_cpu + 0.1), (ang, ang_cpu)
    assert abs(np.linalg.det(F) - 1) < 1e-9


# ---------------------------------------------------------------- evaluate_views
def test_evaluate_views(dev, monkeypatch):
    from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
    from ncnerf_amd.rendering import render
    from ncnerf_amd.synthetic import SyntheticScene
    scene = SyntheticScene()
    torch.manual_seed(0)
    model = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with torch.no_grad():  # a warmed-up occupancy grid
        model.density_grid.copy_(torch.from_numpy(scene.density_grid).to(dev) * 10.0)
        model.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    H, W, V = 96, 128, 2
    dirs = _dev(dir_grid(H, W), dev)
    poses = _dev(scene.poses[:V], dev)
    gts = []
    with torch.no_grad():
        for v in range(V):
            rd = (dirs @ poses[v, :, :3].T).contiguous()
            ro = poses[v, :, 3].expand_as(rd).contiguous()
            gts.append(render(model, ro, rd, near_distance=0.01, max_samples=1024, test_time=True)["rgb"] + 0.1)
    rgb_gt = torch.stack(gts)

    # every way a device tensor reaches the host, recorded (sizes) from the start of evaluate_views
    # until the clustering starts, outside the renderer (whose loop reads its own done flag)
    import ncnerf_amd.rendering as rendering
    copies, watching, renders = [], [True], [0]
    for name in ("cpu", "numpy", "tolist", "item", "__float__", "__int__", "__bool__", "__index__"):
        orig = getattr(torch.Tensor, name)

        def spy(self, *a, _orig=orig, **k):
            if watching[0] and self.is_cuda:
                copies.append(self.numel())
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)
    orig_nc, orig_render = E.normals_clustering, rendering.render

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
    monkeypatch.setattr(E, "normals_clustering", nc_spy)
    monkeypatch.setattr(rendering, "render", render_spy)
    out = E.evaluate_views(model, poses, dirs, (W, H), rgb_gt=rgb_gt, K=30, niter=30, t_similar=0.99,
                           R_ref=torch.eye(3))
    monkeypatch.undo()
    assert renders[0] == V and not watching[0]
    assert copies == [V], copies  # one copy: the V PSNR scalars, after the last view

    assert set(out) == {"psnr", "psnr_mean", "normals", "labels", "centroids", "frame", "angles"}
    assert len(out["psnr"]) == V and all(abs(p - 20.0) <= 1e-3 for p in out["psnr"]), out["psnr"]
    assert abs(out["psnr_mean"] - 20.0) <= 1e-3
    assert out["normals"].shape == (V, H, W, 3) and out["normals"].is_cuda
    n_valid = int(E.valid_normals_mask(out["normals"].reshape(-1, 3)).sum())
    assert out["labels"].shape == (n_valid,) and out["labels"].is_cuda and out["labels"].dtype == torch.int64
    assert out["centroids"].shape == (3, 3) and out["frame"].shape == (3, 3) and out["angles"].shape == (3,)
    assert abs(np.linalg.det(out["frame"]) - 1) < 1e-9
    new, ass, cn = E.normals_clustering(out["normals"], K=30, niter=30, t_similar=0.99, merge_clusters=True,
                                        find_opposite=False)
    assert torch.equal(new, out["labels"]) and torch.equal(cn, out["centroids"])
    assert set(np.unique(new.cpu().numpy()).tolist()) <= {0, 1, 2, 3}
