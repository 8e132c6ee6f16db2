"""The integer label plane of the device data path (ncn_batch_semantics_fw,
DeviceRayDataset(semantics=)): the gather is torch's indexing widened to int64 for uint8, int32 and
int64 planes, an index out of range gives 0 (void), a dataset without the plane draws the batches it
drew, and a batch with it goes through NeRFMTLoss's semantic term."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ncnerf_amd.data import DeviceRayDataset, batch_semantics_fw

pytestmark = pytest.mark.gpu
V, H, W, K = 3, 12, 16, 5  # (16 x 12 images)
BASE_KEYS = {"rays_o", "rays_d", "rgb", "img_idxs", "pix_idxs", "patch_area", "x1_offsets_local", "x2_offsets_local",
             "x3_offsets_local"}


def _plane(dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, K + 1, (V, H * W), generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_gather_is_indexing_widened(dev, dtype, n):
    plane = _plane(dtype)
    if dtype != torch.uint8:
        plane[0, 0], plane[V - 1, H * W - 1] = -3, 2 ** 31 - 1  # signed, and the whole width
    g = torch.Generator().manual_seed(n)
    img, pix = torch.randint(0, V, (n,), generator=g), torch.randint(0, H * W, (n,), generator=g)
    img[0], pix[0] = 0, 0
    img[-1], pix[-1] = (V - 1, H * W - 1) if n > 1 else (0, 0)
    out = torch.full((n,), -7, dtype=torch.int64, device=dev)
    batch_semantics_fw(img.to(dev), pix.to(dev), plane.to(dev), out)
    assert torch.equal(out.cpu(), plane[img, pix].long())


def test_indices_out_of_range_give_void(dev):
    plane = _plane(torch.uint8) + 1  # no zero in the plane
    img = torch.tensor([0, -1, V, 2, 1, 2, 1, 2 ** 40])
    pix = torch.tensor([5, 5, 5, -1, H * W, H * W - 1, 0, 0])
    bad = torch.tensor([False, True, True, True, True, False, False, True])
    out = torch.full((8,), -7, dtype=torch.int64, device=dev)
    batch_semantics_fw(img.to(dev), pix.to(dev), plane.to(dev), out)
    got = out.cpu()
    assert (got[bad] == 0).all() and torch.equal(got[~bad], plane[img[~bad], pix[~bad]].long())
    from ncnerf_amd import _lib
    with pytest.raises(_lib.NcnError, match="plane_bytes = 2"):
        _lib.call("ncn_batch_semantics_fw", img.to(dev), pix.to(dev), 8, plane.to(torch.int16).to(dev), 2, V, H * W, out)
    with pytest.raises(RuntimeError, match="uint8"):
        batch_semantics_fw(img.to(dev), pix.to(dev), plane.to(torch.int16).to(dev), out)


def _dataset(dev, **kw):
    from ncnerf_amd.synthetic import SyntheticScene
    from test_gpu_eval import dir_grid
    scene = SyntheticScene()
    g = torch.Generator().manual_seed(8)
    images = torch.rand(V, H * W, 3, generator=g).to(dev)
    poses = torch.from_numpy(np.ascontiguousarray(scene.poses[:V], dtype=np.float32)).to(dev)
    dirs = torch.from_numpy(np.ascontiguousarray(dir_grid(H, W))).to(dev)
    return scene, DeviceRayDataset(images, poses, dirs, (W, H), batch_size=256, patch_size=8, seed=21, corner_mode="grid",
                                   **kw)


def test_dataset_batches_carry_the_semantics(dev):
    _, plain = _dataset(dev)
    assert set(plain.batch(5)) == BASE_KEYS and plain.semantics is None
    assert set(plain.buffers()) == {"rays_o", "rays_d", "rgb", "img_idxs", "pix_idxs"}
    plane = _plane(torch.uint8).to(dev)
    depth = torch.rand(V, H * W, device=dev)
    _, ds = _dataset(dev, semantics=plane.reshape(V, H, W), depth=depth)
    assert ds.semantics.dtype == torch.uint8 and ds.semantics.shape == (V, H * W) and set(ds.planes) == {"depth"}
    step = torch.tensor(5, dtype=torch.int64, device=dev)
    b = ds.batch(step)
    assert set(b) == BASE_KEYS | {"depth", "semantics"}
    assert b["semantics"].shape == (256,) and b["semantics"].dtype == torch.int64
    assert torch.equal(b["semantics"], plane[b["img_idxs"], b["pix_idxs"]].long())
    assert torch.equal(b["depth"], depth[b["img_idxs"], b["pix_idxs"]])
    ref = plain.batch(step)  # the rays and colours are what a dataset without the plane draws
    for k in ("rays_o", "rays_d", "rgb", "img_idxs", "pix_idxs"):
        assert torch.equal(b[k], ref[k]), k
    bufs = ds.buffers()
    assert set(bufs) == {"rays_o", "rays_d", "rgb", "img_idxs", "pix_idxs", "depth", "semantics"}
    assert set(ds.buffers(labels=False)) == {"rays_o", "rays_d", "rgb", "img_idxs", "pix_idxs"}
    b2 = ds.batch(step, out=bufs)  # written in place: the captured step's static batch
    assert b2["semantics"] is bufs["semantics"] and torch.equal(bufs["semantics"], b["semantics"])
    with pytest.raises(RuntimeError, match="semantics must be a CUDA tensor"):
        _dataset(dev, semantics=plane.cpu())


def test_batch_goes_through_the_semantic_loss_term(dev):
    from ncnerf_amd.losses import NeRFMTLoss
    from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
    from ncnerf_amd.rendering import render
    from ncnerf_amd.trainer import HYPERSIM_HPARAMS
    plane = _plane(torch.int32).to(dev)
    scene, ds = _dataset(dev, semantics=plane)
    torch.manual_seed(7)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128, pred_sem=True, n_sem_cls=K).to(dev))
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-1e-2, 1e-2)
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    b = ds.batch(3)
    loss = NeRFMTLoss(dict(HYPERSIM_HPARAMS, loss_sem_w=0.1, pred_sem=True, load_sem_gt=True, loss_norm_D_C_ort_dot_w=0,
                           loss_norm_D_C_centr_dot_w=0, loss_norm_D_C_centr_L1_w=0))
    noise = torch.rand(256, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    res = render(m, b["rays_o"], b["rays_d"], near_distance=0.01, max_samples=1024, march_noise=noise, n_sem_cls=K)
    ld = loss(res, b, global_step=100)
    want = 0.1 * F.cross_entropy(res["sem"].detach().float(), b["semantics"] - 1, ignore_index=-1)
    np.testing.assert_allclose(float(ld["sem"].detach()), float(want), rtol=1e-5)
    assert float(ld["sem"].detach()) > 0 and int((b["semantics"] == 0).sum()) > 0
