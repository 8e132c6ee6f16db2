"""Torch restatement of the geometry terms of the reference's NeRFMTLoss (losses.py:372-417, with its
validity filter :246-262 and the normals of hypersim_src/utils.py:504-541) — the plain expressions
the package's loss used before these terms moved into ncn_geom_loss_fwd / _bwd.  It runs in the
dtype of its inputs; the tests run it in float64 as the reference of their bounds, and it is itself
held to the reference's own float64 output (tests/golden/geom_losses.npz, tests/test_geom_host.py).

Also the well-conditioned ray patches the fixture and the GPU tests share (patch_rays).
"""
import numpy as np
import torch
import torch.nn.functional as F

KEYS = ("depth", "norm_D_L1", "norm_D_dot", "reg_depth")
RAY_STEP = 0.06  # angular spacing of a patch's rays (radians, at the patch centre)
BOX = 0.5  # the scene box is [-BOX, BOX]^3


def patch_offsets(p=8):
    """The triangle corners of a p x p patch as indices into its cells (base.py:54-58)."""
    o = np.arange(p * p, dtype=np.int64).reshape(p, p)
    return o[1:, 1:].reshape(-1), o[:-1, 1:].reshape(-1), o[1:, :-1].reshape(-1)


def patch_rays(rng, n_patches):
    """n_patches 8x8 patches of rays inside the scene box: per patch a camera position, a viewing
    direction and an 8x8 fan of directions RAY_STEP apart.

    Why not pixel patches of the synthetic scene: the normal of a triangle is a cross product of the
    edges P2 - P1, P3 - P1 of points P = o + d * depth, and in float32 an edge carries a relative
    error of about 2^-24 |P| / |edge|.  Rays one pixel apart (2e-3 rad) give |P| / |edge| ~ 1e3, at
    which float32 autograd of the reference's own expressions is already 1e-4 to 3e-4 (rel. L2) away
    from float64 in d loss / d depth — the bound the tests hold the gradients to.  At RAY_STEP the
    ratio is about 1 / 0.06 ~ 20 and float32 has two orders of magnitude to spare, so what these
    inputs pin is the loss terms, not the conditioning of the normal extraction."""
    o, d = [], []
    iy, ix = np.meshgrid(np.arange(8) - 3.5, np.arange(8) - 3.5, indexing="ij")
    for _ in range(n_patches):
        c = rng.standard_normal(3)
        c /= np.linalg.norm(c)
        u = np.cross(c, [0.0, 0.0, 1.0] if abs(c[2]) < 0.9 else [1.0, 0.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(c, u)
        dirs = c[None] + RAY_STEP * (ix.reshape(-1, 1) * u[None] + iy.reshape(-1, 1) * v[None])
        d.append(dirs / np.linalg.norm(dirs, axis=1, keepdims=True))
        o.append(np.repeat(rng.uniform(-0.2, 0.2, 3)[None], 64, 0))
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)


def box_exit(o, d):
    """(distance to the wall of the scene box along each ray from inside, that wall's normal facing the ray)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (BOX - o) / d, (-BOX - o) / d)
    t = np.where(np.isfinite(t) & (t > 0), t, np.inf)
    ax = t.argmin(axis=1)
    n = np.zeros_like(d)
    n[np.arange(len(ax)), ax] = -np.sign(d[np.arange(len(ax)), ax])
    return t.min(axis=1).astype(np.float32), n.astype(np.float32)


def triangles(n_rays, strategy, offsets=None):
    """x1, x2, x3 (T) int64 ray indices (losses.py:299-313)."""
    if strategy in ("all_images_triang", "same_image_triang"):
        pix = torch.arange(n_rays).reshape(-1, 3)
        return {"x1": pix[:, 0].contiguous(), "x2": pix[:, 1].contiguous(), "x3": pix[:, 2].contiguous()}
    offsets = patch_offsets() if offsets is None else offsets
    area = 64
    pix = torch.arange(n_rays).reshape(-1, area)
    return {k: pix[:, torch.as_tensor(np.asarray(o))].reshape(-1).contiguous() for k, o in zip(("x1", "x2", "x3"), offsets)}


def extract_normals(rays_o, rays_d, depth, x):
    """hypersim_src/utils.py:504-541: normalize(cross(P2 - P1, P3 - P1)), P = o + d * depth."""
    P = rays_o + rays_d * depth[:, None]
    P1, P2, P3 = P[x["x1"]], P[x["x2"]], P[x["x3"]]
    return F.normalize(torch.cross(P2 - P1, P3 - P1, dim=-1), dim=-1)


def _filtered(loss):
    """losses.py:246-262: an empty, NaN or Inf component is replaced by the constant 0."""
    if loss.numel() != 1 or not bool(torch.isfinite(loss)):
        return torch.zeros((), dtype=loss.dtype)
    return loss


def geometry_terms(depth, x, depth_gt=None, normals=None, normals_gt=None, w=(0.0, 0.0, 0.0), reg=False):
    """{key: (filtered loss, weight / count, the mean's addends)} for the terms that are on (a weight
    > 0; reg: the RegNeRF term, past its start).  The addends (a 1-D tensor; the loss before the
    filter is weight / count * addends.sum()) let a test form the fixed-order bound."""
    out = {}
    if w[0] > 0:
        valid = depth_gt > 0
        a = (depth[valid] - depth_gt[valid]) ** 2
        out["depth"] = (_filtered(w[0] * a.mean()), w[0] / max(a.numel(), 1), a.detach().reshape(-1))
    if w[1] > 0 or w[2] > 0:
        tgt = normals_gt[x["x1"]]
        valid = tgt.abs().sum(-1) > 0
        n, g = normals[valid], tgt[valid]
        if w[1] > 0:
            a = (n - g).abs()
            out["norm_D_L1"] = (_filtered(w[1] * a.sum(-1).mean()), w[1] / max(a.shape[0], 1), a.detach().reshape(-1))
        if w[2] > 0:
            a = 1.0 - torch.nn.CosineSimilarity(dim=-1)(n, g)
            out["norm_D_dot"] = (_filtered(w[2] * a.mean()), w[2] / max(a.numel(), 1), a.detach().reshape(-1))
    if reg:
        a = (depth[x["x1"]] - depth[x["x2"]]) ** 2 + (depth[x["x1"]] - depth[x["x3"]]) ** 2
        out["reg_depth"] = (_filtered(a.mean()), 1.0 / max(a.numel(), 1), a.detach().reshape(-1))
    return out


def fixed_order_bound(scale, addends):
    """2 (n - 1) 2^-24 sum|terms| of a mean's n addends, times the mean's factor (weight / count):
    the bound the project holds fixed-order float32 sums to (tests/test_gpu_metrics.py)."""
    n = addends.numel()
    return abs(scale) * 2.0 * max(n - 1, 0) * 2.0 ** -24 * float(addends.double().abs().sum())


class FixtureCase:
    """One case of tests/golden/geom_losses.npz: its inputs as CPU tensors of `dtype`, its settings and
    the reference's results."""

    def __init__(self, f, tag, name, dtype=torch.float64):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        g = lambda k: f[f"{tag}/{name}/{k}"]
        self.strategy = "all_images_triang" if tag == "tri" else "all_images_triang_patch"
        self.variant, self.step, self.start = str(g("variant")), int(g("step")), int(g("loss_norm_can_start"))
        self.w = tuple(float(g(k)) for k in ("loss_depth_w", "loss_norm_depth_L1_w", "loss_norm_depth_dot_w"))
        self.reg_w = float(g("loss_reg_depth_w"))
        self.gt_depth = bool(g("loss_norm_GT_depth"))
        depth = f[f"{tag}/depth"].copy()
        depth_gt, normals, normals_depth = (f[f"{tag}/{k}"] for k in ("depth_gt", "normals_gt", "normals_depth_gt"))
        if self.variant == "empty":
            depth_gt, normals, normals_depth = (np.zeros_like(a) for a in (depth_gt, normals, normals_depth))
        if self.variant == "nan":
            depth[int(f[f"{tag}/nan_ray"])] = np.nan
        self.depth, self.rays_o, self.rays_d = t(depth), t(f[f"{tag}/rays_o"]), t(f[f"{tag}/rays_d"])
        self.rgb_pred, self.rgb_gt = t(f[f"{tag}/rgb_pred"]), t(f[f"{tag}/rgb_gt"])
        self.depth_gt, self.normals, self.normals_depth = t(depth_gt), t(normals), t(normals_depth)
        self.offsets = None
        if tag == "patch":
            self.offsets = tuple(f[f"{tag}/{k}_offsets_local"] for k in ("x1", "x2", "x3"))
        self.x = triangles(len(depth), self.strategy, self.offsets)
        self.keys = [str(k) for k in g("keys")]
        self.loss32 = {k: float(g("loss_" + k)) for k in self.keys}
        self.loss64 = {k: float(g("loss64_" + k)) for k in self.keys}
        self.grad32, self.grad64 = g("grad_depth"), g("grad_depth64")

    def hparams(self):
        """The NeRFMTLoss settings of the case (everything else off)."""
        return dict(loss_opacity_w=0, loss_depth_w=self.w[0], loss_norm_depth_L1_w=self.w[1],
                    loss_norm_depth_dot_w=self.w[2], loss_reg_depth_w=self.reg_w, loss_norm_GT_depth=self.gt_depth,
                    loss_norm_can_start=self.start, loss_norm_can_end=-1, loss_norm_can_grow=2500,
                    ray_sampling_strategy=self.strategy, pred_norm_depth=True)

    def expected_keys(self):
        """The geometry entries this package returns: the reference's, with its `norm` entry (an empty
        normal mask, losses.py:408) as the two terms' own zeros."""
        keys = set(self.keys) - {"rgb", "total"}
        if "norm" in keys:
            keys = keys - {"norm"} | {"norm_D_L1", "norm_D_dot"}
        return keys

    def restated(self):
        """(terms of geometry_terms, d sum(terms) / d depth) in this case's dtype."""
        depth = self.depth.clone().requires_grad_(True)
        normals = extract_normals(self.rays_o, self.rays_d, depth, self.x)
        terms = geometry_terms(depth, self.x, self.depth_gt, normals, self.normals_depth if self.gt_depth else self.normals,
                               self.w, self.reg_w > 0 and self.step > self.start)
        total = sum(v[0] for v in terms.values())
        grad = torch.zeros_like(self.depth)
        if isinstance(total, torch.Tensor) and total.requires_grad:
            grad = torch.autograd.grad(total, depth)[0]
        return terms, grad
