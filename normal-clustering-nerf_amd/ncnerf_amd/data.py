"""The training set in device memory: batches are drawn and their rays generated on the device.

Replaces, per training step, BaseDataset.__getitem__ (datasets/base.py:142-182: numpy draws and a
gather from the host image stack), the host-to-device copy of the batch, and the ray code of
NeRFSystem.forward (train_nerf.py:167-182: poses[img_idxs], directions[pix_idxs], axisangle_to_R,
get_rays) by two launches — ncn_batch_draw and ncn_batch_rays_fw — that read nothing from the host
but a step counter, which may itself live on the device: with preallocated outputs they can be
captured in a HIP graph.  A dataset that was given label planes (depth, normals, normals_depth: the
targets of NeRFMTLoss's depth and GT-normal terms) gathers them for the drawn rays in a third launch,
ncn_batch_labels_fw, and its batches carry them under those keys; a `semantics` plane of integer
class labels (the target of NeRFMTLoss's semantic term and of the semantic metrics; 0 = void) is
gathered behind it by ncn_batch_semantics_fw into int64 labels.  The batch is the dict
Trainer.step(batch, ...) takes, and Trainer.step_from(dataset, step) / Trainer.fit(dataset, n_steps)
draw it themselves: the captured step begins with batch(device step counter, out=its static
buffers, seed=seed + rank), so the launches above are nodes of its graph (trainer.py).
With optimize_ext the dataset holds the reference's per-image pose corrections dR (axis-angle) and dT
(train_nerf.py:244-249) and the rays carry their gradient (ncn_batch_rays_bw, deterministic); the
eager step_from steps them (optim.PoseAdam).

Only the two patch strategies are implemented (`all_images_triang_patch`, `same_image_triang_patch`).
The draws are counter-based (seed, step, patch), not numpy's global generator.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call

STRATEGIES = ("all_images_triang_patch", "same_image_triang_patch")
CORNER_MODES = {"reference": _lib.CONSTANTS["NCN_CORNER_REFERENCE"], "grid": _lib.CONSTANTS["NCN_CORNER_GRID"]}
_IMAGE_DTYPES = {torch.float32: _lib.CONSTANTS["NCN_IMAGE_F32"], torch.uint8: _lib.CONSTANTS["NCN_IMAGE_U8"]}


def patch_offsets(patch_size):
    """The triangle corners of a patch as indices into its patch_size^2 cells (base.py:54-58)."""
    o = np.arange(patch_size * patch_size, dtype=np.int64).reshape(patch_size, patch_size)
    return o[1:, 1:].reshape(-1), o[:-1, 1:].reshape(-1), o[1:, :-1].reshape(-1)


def batch_draw(seed, step, n_images, H, W, patch, n_patches, same_image, corner_mode, img_idxs, pix_idxs):
    """ncn_batch_draw into img_idxs / pix_idxs (int64 CUDA, n_patches * patch^2).  step: an int, or a
    device int64 scalar (read by the kernel: no host read)."""
    if isinstance(step, torch.Tensor):
        _lib.check_input(step, "step")
        _lib.check_dtype(step, torch.int64, "step")
        step_dev, step_host = step, 0
    else:
        step_dev, step_host = None, int(step)
    call("ncn_batch_draw", int(seed) & (2 ** 64 - 1), step_dev, step_host, n_images, H, W,
         patch, n_patches, 1 if same_image else 0, corner_mode, img_idxs, pix_idxs)


def batch_rays_fw(img_idxs, pix_idxs, images, directions, poses, dR, dT, rays_o, rays_d, rgb):
    """ncn_batch_rays_fw; dR = dT = None: the stored poses."""
    call("ncn_batch_rays_fw", img_idxs, pix_idxs, img_idxs.numel(), images, _IMAGE_DTYPES[images.dtype], directions,
         poses, dR, dT, poses.shape[0], directions.shape[0], rays_o, rays_d, rgb)


def batch_rays_bw(g_o, g_d, img_idxs, pix_idxs, directions, poses, dR, grad_dR, grad_dT):
    """ncn_batch_rays_bw: every row of grad_dR / grad_dT (V,3) is written."""
    call("ncn_batch_rays_bw", g_o, g_d, img_idxs, pix_idxs, img_idxs.numel(), directions, poses, dR, poses.shape[0],
         directions.shape[0], grad_dR, grad_dT)


LABEL_PLANES = ("depth", "normals", "normals_depth")  # their widths: 1, 3, 3


def batch_labels_fw(img_idxs, pix_idxs, planes, out):
    """ncn_batch_labels_fw: out[k][r] = planes[k][img_idxs[r], pix_idxs[r]] for the planes that are there
    (dicts keyed by LABEL_PLANES; depth (V, H*W), normals / normals_depth (V, H*W, 3)); an index out
    of range gives NaN."""
    given = [planes[k] for k in LABEL_PLANES if planes.get(k) is not None]
    if not given:
        return
    call("ncn_batch_labels_fw", img_idxs, pix_idxs, img_idxs.numel(), planes.get("depth"), planes.get("normals"),
         planes.get("normals_depth"), given[0].shape[0], given[0].shape[1],
         *(out[k] if planes.get(k) is not None else None for k in LABEL_PLANES))


_SEMANTICS_DTYPES = (torch.uint8, torch.int32, torch.int64)  # the widths ncn_batch_semantics_fw takes: 1, 4, 8


def batch_semantics_fw(img_idxs, pix_idxs, plane, out):
    """ncn_batch_semantics_fw: out[r] = plane[img_idxs[r], pix_idxs[r]] as int64 for plane (V, H*W) uint8,
    int32 or int64; an index out of range gives 0 (void)."""
    if plane.dtype not in _SEMANTICS_DTYPES:
        raise RuntimeError(f"semantics must be torch.uint8, torch.int32 or torch.int64 (got {plane.dtype})")
    call("ncn_batch_semantics_fw", img_idxs, pix_idxs, img_idxs.numel(), plane, plane.element_size(), plane.shape[0],
         plane.shape[1], out)


class _PoseRays(torch.autograd.Function):
    """rays_o, rays_d, rgb of a drawn batch as a function of dR, dT (train_nerf.py:177-182)."""

    @staticmethod
    def forward(ctx, dR, dT, ds, img_idxs, pix_idxs, rays_o, rays_d, rgb):
        batch_rays_fw(img_idxs, pix_idxs, ds.images, ds.directions, ds.poses, dR, dT, rays_o, rays_d, rgb)
        ctx.ds = ds
        ctx.save_for_backward(dR, img_idxs, pix_idxs)
        ctx.mark_dirty(rays_o, rays_d, rgb)
        ctx.mark_non_differentiable(rgb)
        return rays_o, rays_d, rgb

    @staticmethod
    def backward(ctx, g_o, g_d, _g_rgb):
        dR, img_idxs, pix_idxs = ctx.saved_tensors
        ds = ctx.ds
        n = img_idxs.numel()
        g_o = torch.zeros(n, 3, device=dR.device) if g_o is None else g_o.contiguous().float()
        g_d = torch.zeros(n, 3, device=dR.device) if g_d is None else g_d.contiguous().float()
        grad_dR, grad_dT = torch.empty_like(dR), torch.empty_like(dR)
        batch_rays_bw(g_o, g_d, img_idxs, pix_idxs, ds.directions, ds.poses, dR, grad_dR, grad_dT)
        return grad_dR, grad_dT, None, None, None, None, None, None


class DeviceRayDataset:
    """images (V, H*W, 3) or (V, H, W, 3), float32 in [0, 1] or uint8; poses (V, 3, 4) camera-to-world;
    directions (H*W, 3) camera-space ray directions (get_ray_directions); img_wh = (W, H) as the
    reference's datasets keep it.  corner_mode "reference" keeps base.py:164-166's pixel arithmetic
    (DESIGN.md §3), "grid" draws patches that lie inside the image.  depth (V, H*W) or (V, H, W),
    normals and normals_depth (V, H*W, 3) or (V, H, W, 3), float32: optional label planes, gathered
    into every batch under their names.  semantics (V, H*W) or (V, H, W), uint8, int32 or int64 (kept
    in its dtype): optional raw class labels, 0 = void, gathered into every batch as "semantics" (n) int64."""

    def __init__(self, images, poses, directions, img_wh, batch_size=8192, patch_size=8,
                 ray_sampling_strategy="all_images_triang_patch", seed=0, corner_mode="reference", optimize_ext=False,
                 depth=None, normals=None, normals_depth=None, semantics=None):
        if ray_sampling_strategy not in STRATEGIES:
            raise ValueError(f"ray_sampling_strategy {ray_sampling_strategy!r} is not implemented on the device; "
                             f"one of {STRATEGIES}")
        if corner_mode not in CORNER_MODES:
            raise ValueError(f"corner_mode {corner_mode!r}; one of {sorted(CORNER_MODES)}")
        planes = {k: t for k, t in zip(LABEL_PLANES, (depth, normals, normals_depth)) if t is not None}
        for t, name in ((images, "images"), (poses, "poses"), (directions, "directions")) + tuple(
                (t, k) for k, t in planes.items()) + (((semantics, "semantics"),) if semantics is not None else ()):
            if not isinstance(t, torch.Tensor):
                raise RuntimeError(f"{name} must be a CUDA tensor")
        W, H = int(img_wh[0]), int(img_wh[1])
        if W < 1 or H < 1:
            raise ValueError(f"img_wh {tuple(img_wh)}")
        if images.dtype not in _IMAGE_DTYPES:
            raise RuntimeError(f"images must be torch.float32 or torch.uint8 (got {images.dtype})")
        _lib.check_dtype(poses, torch.float32, "poses")
        _lib.check_dtype(directions, torch.float32, "directions")
        if images.dim() == 4:
            images = images.reshape(images.shape[0], -1, images.shape[-1])
        V = images.shape[0]
        if V < 1:
            raise ValueError("the dataset needs at least one image")
        if tuple(images.shape) != (V, H * W, 3):
            raise ValueError(f"images must be (V, {H * W}, 3) for img_wh {(W, H)} (got {tuple(images.shape)})")
        if tuple(poses.shape) != (V, 3, 4):
            raise ValueError(f"poses must be ({V}, 3, 4) (got {tuple(poses.shape)})")
        if tuple(directions.shape) != (H * W, 3):
            raise ValueError(f"directions must be ({H * W}, 3) (got {tuple(directions.shape)})")
        for k, t in planes.items():
            _lib.check_dtype(t, torch.float32, k)
            shape = (V, H * W) if k == "depth" else (V, H * W, 3)
            full = (V, H, W) if k == "depth" else (V, H, W, 3)
            if tuple(t.shape) == full:
                planes[k] = t = t.reshape(shape)
            if tuple(t.shape) != shape:
                raise ValueError(f"{k} must be {shape} for img_wh {(W, H)} (got {tuple(t.shape)})")
        if semantics is not None:
            if semantics.dtype not in _SEMANTICS_DTYPES:
                raise RuntimeError(f"semantics must be torch.uint8, torch.int32 or torch.int64 (got {semantics.dtype})")
            if tuple(semantics.shape) == (V, H, W):
                semantics = semantics.reshape(V, H * W)
            if tuple(semantics.shape) != (V, H * W):
                raise ValueError(f"semantics must be {(V, H * W)} for img_wh {(W, H)} (got {tuple(semantics.shape)})")
        patch_size, batch_size = int(patch_size), int(batch_size)
        if patch_size < 1 or patch_size > min(H, W):
            raise ValueError(f"patch_size {patch_size} does not fit a {W}x{H} image")
        if batch_size < 1 or batch_size % (patch_size * patch_size) != 0:
            raise ValueError(f"batch_size {batch_size} is not a multiple of patch_size^2 = {patch_size * patch_size}")
        # (the device last, so every check above also runs — and is tested — on a host without a GPU)
        for t, name in ((images, "images"), (poses, "poses"), (directions, "directions")) + tuple(
                (t, k) for k, t in planes.items()):
            _lib.check_input(t, name)
        if not (images.device == poses.device == directions.device):
            raise RuntimeError("images, poses and directions must be on one device")
        for k, t in planes.items():
            if t.device != images.device:
                raise RuntimeError(f"{k} must be on the device of images")
        if semantics is not None:
            _lib.check_input(semantics, "semantics")
            if semantics.device != images.device:
                raise RuntimeError("semantics must be on the device of images")
        self.images, self.poses, self.directions = images, poses, directions
        self.planes = planes  # the label planes that were given, by name
        self.semantics = semantics  # the integer label plane, or None (not one of LABEL_PLANES: another gather)
        self.H, self.W, self.n_images = H, W, V
        self.batch_size, self.patch_size = batch_size, patch_size
        self.n_patches = batch_size // (patch_size * patch_size)
        self.ray_sampling_strategy = ray_sampling_strategy
        self.same_image = ray_sampling_strategy == "same_image_triang_patch"
        self.corner_mode = CORNER_MODES[corner_mode]
        self.seed = int(seed)
        self.device = images.device
        self.x1_off, self.x2_off, self.x3_off = patch_offsets(patch_size)
        self.optimize_ext = bool(optimize_ext)
        self.dR = self.dT = None
        if self.optimize_ext:  # train_nerf.py:244-249
            self.dR = torch.nn.Parameter(torch.zeros(V, 3, device=self.device))
            self.dT = torch.nn.Parameter(torch.zeros(V, 3, device=self.device))

    def buffers(self, n_rays=None, labels=True):
        """Preallocated outputs of batch(out=...): the static batch buffers of a captured step, with
        one buffer per label plane of the dataset (the semantics included) unless labels is False."""
        n = self.batch_size if n_rays is None else n_rays
        f = dict(dtype=torch.float32, device=self.device)
        i = dict(dtype=torch.int64, device=self.device)
        out = {"rays_o": torch.empty(n, 3, **f), "rays_d": torch.empty(n, 3, **f), "rgb": torch.empty(n, 3, **f),
               "img_idxs": torch.empty(n, **i), "pix_idxs": torch.empty(n, **i)}
        for k in (self.planes if labels else ()):
            out[k] = torch.empty((n,) if k == "depth" else (n, 3), **f)
        if labels and self.semantics is not None:
            out["semantics"] = torch.empty(n, **i)
        return out

    def _rays(self, img_idxs, pix_idxs, out):
        if self.optimize_ext and torch.is_grad_enabled():
            # (fresh views of the buffers: a reused buffer must not carry the previous batch's history)
            return _PoseRays.apply(self.dR, self.dT, self, img_idxs, pix_idxs, out["rays_o"].detach(),
                                   out["rays_d"].detach(), out["rgb"].detach())
        dR = self.dR.detach() if self.optimize_ext else None
        dT = self.dT.detach() if self.optimize_ext else None
        batch_rays_fw(img_idxs, pix_idxs, self.images, self.directions, self.poses, dR, dT, out["rays_o"],
                      out["rays_d"], out["rgb"])
        return out["rays_o"], out["rays_d"], out["rgb"]

    def batch(self, step, out=None, seed=None):
        """The batch of `step` (an int or a device int64 scalar) as the dict Trainer.step and NeRFMTLoss
        take.  out: buffers() to write into (nothing is allocated: capturable); seed: overrides the
        dataset's (data-parallel ranks draw with seed + rank).  No host read either way.  The label
        planes the dataset holds come with it under "depth" (n), "normals", "normals_depth" (n, 3),
        "semantics" (n) int64."""
        out = self.buffers() if out is None else out
        batch_draw(self.seed if seed is None else seed, step, self.n_images, self.H, self.W, self.patch_size,
                   self.n_patches, self.same_image, self.corner_mode, out["img_idxs"], out["pix_idxs"])
        rays_o, rays_d, rgb = self._rays(out["img_idxs"], out["pix_idxs"], out)
        batch = {"rays_o": rays_o, "rays_d": rays_d, "rgb": rgb, "img_idxs": out["img_idxs"],
                 "pix_idxs": out["pix_idxs"], "patch_area": self.patch_size * self.patch_size,
                 "x1_offsets_local": self.x1_off, "x2_offsets_local": self.x2_off, "x3_offsets_local": self.x3_off}
        if self.planes:  # (one launch for all of them)
            batch_labels_fw(out["img_idxs"], out["pix_idxs"], self.planes, out)
            batch.update((k, out[k]) for k in self.planes)
        if self.semantics is not None:
            batch_semantics_fw(out["img_idxs"], out["pix_idxs"], self.semantics, out["semantics"])
            batch["semantics"] = out["semantics"]
        return batch

    def image_rays(self, v):
        """Every pixel of view v — rays_o, rays_d, rgb (H*W, 3) — through the same forward kernel (with
        the refined pose under optimize_ext, no gradient): the rays evaluate_views takes."""
        if not 0 <= int(v) < self.n_images:
            raise IndexError(f"view {v} of {self.n_images}")
        n = self.H * self.W
        out = self.buffers(n, labels=False)
        out["img_idxs"].fill_(int(v))
        torch.arange(n, out=out["pix_idxs"])
        with torch.no_grad():
            return self._rays(out["img_idxs"], out["pix_idxs"], out)
