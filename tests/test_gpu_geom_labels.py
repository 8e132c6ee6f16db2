"""Label planes of the device data path (ncn_batch_labels_fw, DeviceRayDataset(depth=, normals=,
normals_depth=)): the gather is numpy's indexing exactly, an index out of range gives NaN, a missing
plane is skipped, and the dataset's batches carry the planes it was given — and only those."""
import numpy as np
import pytest
import torch

import data_ref
from ncnerf_amd.data import DeviceRayDataset, batch_labels_fw
from ncnerf_amd.synthetic import make_cameras

pytestmark = pytest.mark.gpu
V, H, W = 5, 20, 24


def _planes(dev, seed=3):
    rng = np.random.default_rng(seed)
    host = {"depth": rng.random((V, H * W), dtype=np.float32) + 0.5,
            "normals": rng.standard_normal((V, H * W, 3)).astype(np.float32),
            "normals_depth": rng.standard_normal((V, H * W, 3)).astype(np.float32)}
    return host, {k: torch.from_numpy(v).to(dev) for k, v in host.items()}


def _out(dev, n, fill=-7.0):
    return {"depth": torch.full((n,), fill, device=dev), "normals": torch.full((n, 3), fill, device=dev),
            "normals_depth": torch.full((n, 3), fill, device=dev)}


# 300 rays: a partial second workgroup; 1: a single thread
@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("given", [("depth", "normals", "normals_depth"), ("depth",), ("normals_depth",),
                                   ("normals", "normals_depth")])
def test_gather_is_numpy_indexing(dev, n, given):
    host, planes = _planes(dev)
    rng = np.random.default_rng(n)
    img, pix = rng.integers(0, V, n), rng.integers(0, H * W, n)
    out = _out(dev, n)
    batch_labels_fw(torch.from_numpy(img).to(dev), torch.from_numpy(pix).to(dev), {k: planes[k] for k in given}, out)
    torch.cuda.synchronize()
    for k in host:
        got = out[k].cpu().numpy()
        if k in given:
            assert np.array_equal(got, host[k][img, pix]), k
        else:
            assert (got == -7.0).all(), k  # a plane that is not there: its output is left alone


def test_indices_out_of_range_give_nan(dev):
    host, planes = _planes(dev)
    img = np.array([0, -1, V, 2, 3, 4, 1, 2 ** 40], np.int64)
    pix = np.array([5, 5, 5, -1, H * W, H * W - 1, 0, 0], np.int64)
    bad = np.array([False, True, True, True, True, False, False, True])
    out = _out(dev, 8)
    batch_labels_fw(torch.from_numpy(img).to(dev), torch.from_numpy(pix).to(dev), planes, out)
    torch.cuda.synchronize()
    for k in host:
        got = out[k].cpu().numpy()
        assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], host[k][img[~bad], pix[~bad]]), k


def _dataset(dev, planes, **kw):
    images, _, directions = data_ref.small_scene(V, H, W, seed=6)
    return DeviceRayDataset(torch.from_numpy(images).to(dev), torch.from_numpy(make_cameras(V, seed=2)).to(dev),
                            torch.from_numpy(directions).to(dev), (W, H), batch_size=256, seed=21, **planes, **kw)


def test_dataset_batches_carry_the_planes(dev):
    host, planes = _planes(dev)
    plain = _dataset(dev, {})
    base_keys = {"rays_o", "rays_d", "rgb", "img_idxs", "pix_idxs", "patch_area", "x1_offsets_local", "x2_offsets_local",
                 "x3_offsets_local"}
    assert set(plain.batch(5)) == base_keys
    assert set(plain.buffers()) == {"rays_o", "rays_d", "rgb", "img_idxs", "pix_idxs"}
    # every plane, one of them given as (V, H, W, 3)
    ds = _dataset(dev, dict(planes, normals=planes["normals"].reshape(V, H, W, 3)))
    step = torch.tensor(5, dtype=torch.int64, device=dev)
    b = ds.batch(step)
    assert set(b) == base_keys | {"depth", "normals", "normals_depth"}
    assert b["depth"].shape == (256,) and b["normals"].shape == b["normals_depth"].shape == (256, 3)
    img, pix = b["img_idxs"], b["pix_idxs"]
    for k in host:
        assert torch.equal(b[k], planes[k][img, pix]), k
    ref = plain.batch(step)  # the rays and colours are what a dataset without planes draws
    for k in ("rays_o", "rays_d", "rgb", "img_idxs", "pix_idxs"):
        assert torch.equal(b[k], ref[k]), k
    # preallocated buffers are written in place (the captured step's static batch)
    bufs = ds.buffers()
    assert set(bufs) == {"rays_o", "rays_d", "rgb", "img_idxs", "pix_idxs", "depth", "normals", "normals_depth"}
    b2 = ds.batch(step, out=bufs)
    assert b2["depth"] is bufs["depth"] and torch.equal(bufs["normals_depth"], b["normals_depth"])
    # only the planes that were given
    only = _dataset(dev, {"normals_depth": planes["normals_depth"]})
    b3 = only.batch(5)
    assert set(b3) == base_keys | {"normals_depth"} and torch.equal(b3["normals_depth"], b["normals_depth"])


def test_full_view_gather_is_the_plane(dev):
    """image_rays-style indexing (img_idxs = v, pix_idxs = 0 .. H*W - 1) returns view v of every plane;
    image_rays itself is unchanged: three (H*W, 3) tensors."""
    host, planes = _planes(dev)
    ds = _dataset(dev, planes)
    v = 3
    out = ds.buffers(H * W)
    out["img_idxs"].fill_(v)
    torch.arange(H * W, out=out["pix_idxs"])
    batch_labels_fw(out["img_idxs"], out["pix_idxs"], ds.planes, out)
    for k in host:
        assert torch.equal(out[k], planes[k][v]), k
    rays = ds.image_rays(v)
    assert len(rays) == 3 and all(t.shape == (H * W, 3) for t in rays)


def test_planes_on_another_device_are_refused(dev):
    host, planes = _planes(dev)
    with pytest.raises(RuntimeError, match="depth must be a CUDA tensor"):
        _dataset(dev, {"depth": torch.from_numpy(host["depth"])})
