"""The device data path on a host without a GPU: the module's surface, the restated sampler
(tests/data_ref.py) against the reference's literal pixel arithmetic, the uniformity of the restated
draws (the device is held bit-equal to the restatement in tests/test_gpu_data.py, so it needs no
distribution test of its own), and DeviceRayDataset's argument checks."""
import numpy as np
import pytest
import torch

import data_ref

SHAPES = [(768, 1024, 8), (8, 9, 8), (5, 7, 2), (4, 4, 4)]


def test_module_is_part_of_the_package():
    import ncnerf_amd
    from ncnerf_amd import data
    assert "data" in ncnerf_amd.__all__
    assert hasattr(data, "DeviceRayDataset")


@pytest.mark.parametrize("H,W,p", SHAPES)
def test_reference_corner_mode_is_the_literal_arithmetic(H, W, p):
    """base.py:44-62, 164-166: ordinals[:, None] + img_idx[:p, :p].reshape(-1)[None]."""
    n_corners = (H - p + 1) * (W - p + 1)
    ordinals = np.arange(n_corners, dtype=np.int64)
    img_idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    literal = ordinals[:, None] + img_idx[:p, :p].reshape(-1)[None]
    got = data_ref.patch_pixels(ordinals, H, W, p, "reference")
    assert np.array_equal(got, literal)
    assert got.min() == 0 and got.max() == H * W - 1 - (p - 1) * (H - p) < H * W


@pytest.mark.parametrize("H,W,p", SHAPES)
def test_grid_corner_mode_stays_inside_rows(H, W, p):
    n_corners = (H - p + 1) * (W - p + 1)
    pix = data_ref.patch_pixels(np.arange(n_corners), H, W, p, "grid").reshape(n_corners, p, p)
    rows, cols = pix // W, pix % W
    assert pix.min() == 0 and pix.max() == H * W - 1
    assert (rows == rows[:, :, :1]).all() and (np.diff(rows, axis=1) == 1).all()  # one image row per patch row
    assert (np.diff(cols, axis=2) == 1).all() and (cols == cols[:, :1, :]).all()
    # every corner of the image's corner grid exactly once
    assert len({(int(r), int(c)) for r, c in zip(rows[:, 0, 0], cols[:, 0, 0])}) == n_corners


def test_draws_are_uniform():
    """16384 patches, 5 images, 24x20 pixels, patch 8 (221 corners): chi-square of the image and the
    corner counts below the 99.9 % quantile, over fixed (seed, step) pairs (deterministic)."""
    from scipy.stats import chi2
    n, V, H, W, p = 16384, 5, 20, 24, 8
    n_corners = (H - p + 1) * (W - p + 1)
    assert n_corners == 221
    q_img, q_cor = chi2.ppf(0.999, V - 1), chi2.ppf(0.999, n_corners - 1)
    assert abs(q_img - 18.47) < 0.01
    for seed, step in ((0, 0), (1, 7), (12345, 2 ** 32 + 3)):
        imgs, corners = data_ref.draw_patches(seed, step, V, H, W, p, n, same_image=False)
        assert 0 <= imgs.min() and imgs.max() < V and 0 <= corners.min() and corners.max() < n_corners
        for x, k, q in ((imgs, V, q_img), (corners, n_corners, q_cor)):
            cnt = np.bincount(x, minlength=k).astype(np.float64)
            stat = float(((cnt - n / k) ** 2 / (n / k)).sum())
            print(f"seed {seed} step {step}: chi2({k - 1}) = {stat:.2f} (limit {q:.2f})")
            assert stat < q
        # the two streams of a patch are not the same draw
        assert abs(np.corrcoef(imgs / V, corners / n_corners)[0, 1]) < 0.05
    # same_image: one image for the whole batch, changing with the step
    one = [data_ref.draw_patches(3, s, V, H, W, p, 16, same_image=True)[0] for s in range(64)]
    assert all(len(set(o.tolist())) == 1 for o in one)
    assert len({int(o[0]) for o in one}) == V


def test_fp64_gradient_at_zero_rotation_is_finite():
    """The backward's reference at dR = 0: torch's norm has the subgradient 0 there."""
    v = torch.zeros(2, 3, dtype=torch.float64, requires_grad=True)
    g = torch.arange(18, dtype=torch.float64).reshape(2, 3, 3)
    (data_ref.axis_angle_matrix(v) * g).sum().backward()
    assert bool(torch.isfinite(v.grad).all())
    # d A / d v_k at 0 is skew(e_k) (sin t / t -> 1): <g, E_0> = g[2,1] - g[1,2]
    assert torch.allclose(v.grad[0], torch.stack([g[0, 2, 1] - g[0, 1, 2], g[0, 0, 2] - g[0, 2, 0],
                                                  g[0, 1, 0] - g[0, 0, 1]]), rtol=1e-6)


def _args(V=2, H=8, W=9):
    images, poses, directions = data_ref.small_scene(V, H, W)
    return torch.from_numpy(images), torch.from_numpy(poses), torch.from_numpy(directions), (W, H)


def test_dataset_argument_checks():
    from ncnerf_amd.data import DeviceRayDataset
    im, po, di, wh = _args()
    ok = dict(batch_size=64, patch_size=8)
    for strategy in ("all_images", "same_image", "all_images_triang", "same_image_triang", "random_tr_poses"):
        with pytest.raises(ValueError, match="ray_sampling_strategy"):
            DeviceRayDataset(im, po, di, wh, ray_sampling_strategy=strategy, **ok)
    with pytest.raises(ValueError, match="corner_mode"):
        DeviceRayDataset(im, po, di, wh, corner_mode="wrapped", **ok)
    with pytest.raises(ValueError, match="multiple of patch_size"):
        DeviceRayDataset(im, po, di, wh, batch_size=100, patch_size=8)
    with pytest.raises(ValueError, match="does not fit"):
        DeviceRayDataset(im, po, di, wh, batch_size=81, patch_size=9)
    with pytest.raises(ValueError, match="at least one image"):
        DeviceRayDataset(im[:0], po[:0], di, wh, **ok)
    with pytest.raises(ValueError, match="images must be"):
        DeviceRayDataset(im[:, :-1], po, di, wh, **ok)
    with pytest.raises(ValueError, match="poses must be"):
        DeviceRayDataset(im, po[:1], di, wh, **ok)
    with pytest.raises(ValueError, match="directions must be"):
        DeviceRayDataset(im, po, di[:-1], wh, **ok)
    with pytest.raises(RuntimeError, match="images must be torch.float32 or torch.uint8"):
        DeviceRayDataset(im.double(), po, di, wh, **ok)
    with pytest.raises(RuntimeError, match="poses must be"):
        DeviceRayDataset(im, po.double(), di, wh, **ok)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        DeviceRayDataset(im.numpy(), po, di, wh, **ok)


def test_cpu_tensors_are_refused_before_any_library_call(monkeypatch):
    from ncnerf_amd import _lib
    from ncnerf_amd.data import DeviceRayDataset

    def no_call(name, *a):
        raise AssertionError(f"library call {name} with CPU tensors")

    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr("ncnerf_amd.data.call", no_call)
    im, po, di, wh = _args()
    with pytest.raises(RuntimeError, match="images must be a CUDA tensor"):
        DeviceRayDataset(im, po, di, wh, batch_size=64, patch_size=8)
    with pytest.raises(RuntimeError, match="images must be a CUDA tensor"):
        DeviceRayDataset(im, po, di, wh, batch_size=64, patch_size=8, optimize_ext=True)
