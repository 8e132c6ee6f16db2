"""NeRFMTLoss of the reference losses.py:169-587 for the training hot path.

Kept: the photometric MSE (losses.py:349-355), opacity entropy (:358-362), depth L2 (:372-385),
normals-from-depth vs GT normals L1/dot (:388-411), RegNeRF depth smoothness (:414-418) and the
normal-clustering block (:420-509) with its weight schedule (:217) and validity filter (:246-262).
The clustering block runs on the GPU end to end: `_extract_normals_from_ray_batch`
(hypersim_src/utils.py:504-541) is `ncn_normals_fwd/bwd`, and faiss k-means + the cluster selection
+ the three cluster losses + their gradient are ONE persistent launch (`ncn_cluster_loss`), so the
step no longer copies normals to the host (losses.py:434) or syncs on `.item()`s.

The k-means restates faiss's published `Clustering::train` as losses.py:86-89 calls it
(faiss.Kmeans(3, 20, niter=20, spherical=True)): the training set subsampled to 256*K points by
rand_perm(seed 1234) when larger, the initial centroids the first K of rand_perm(seed 1235), Lloyd
rounds with spherical renormalisation and faiss's split_clusters for empty clusters (its
RandomGenerator walk from a host-built std::mt19937 plan), then a final search over all points.
faiss itself is not available here: parity unpinned w.r.t. faiss, see DESIGN.md §3.

The geometry supervision — depth L2, the two GT-normal terms and RegNeRF — is one autograd node
(`_GeomLoss`) over two entry points, `ncn_geom_loss_fwd` / `ncn_geom_loss_bwd` (include/ncnerf_geom.h):
masks, fixed-order sums, the validity filter and the RegNeRF step gate all stay on the device, so
these terms run inside a captured step (a device `global_step`) like the rest.  The normal terms'
gradient is carried through the triangle normals to the depth inside the backward launch, which
skips every triangle of a filtered term: the reference replaces such a term by a constant, so no
0 * NaN of a NaN depth may reach the gradient.  Only under pose refinement (the rays require grad)
does it go on as dL/dnormals into `_Normals.backward`, which also reaches the rays.

Pose refinement (train_nerf.py --optimize_ext: the prediction's rays require grad): `_Normals`
back-propagates into rays_o / rays_d (`ncn_normals_bwd_rays`), NeRFMTLoss.forward then takes the
unfused `_Normals` + `cluster_losses` branch, and the fused nodes, which stop at the depth, raise.

The semantic term (losses.py:568-573; `loss_sem_w > 0` with `pred_sem` and `load_sem_gt` in the
hyper-parameters, as the reference asserts): loss_sem_w * CE(pred['sem'][:gt_l], target['semantics'] - 1,
ignore_index=-1), label 0 = void.  It stays on the device (torch's cross_entropy, summed and divided
by the clamped count of labelled rays, no host read: capturable); a batch whose labels are all void
gives exactly 0 and exactly zero gradients, where the reference's mean over no element is the NaN
its validity filter replaces by 0.

Not provided (weight 0 in every reference config, hyperparameters.py:33-49): the Manhattan-NeRF and
canonical-direction terms (raise if enabled; the reference's own asserts, losses.py:227-231, make its
Manhattan-NeRF branch unreachable).
"""
import einops
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, vren
from ._lib import call, check_input

N_OUT = 11  # ncn_cluster_loss out_losses
K_CLUSTERS, K_ITERS = 20, 20  # losses.py:86-89: faiss.Kmeans(3, 20, niter=20)
_WS = {}


def _cluster_workspace(dev, K):
    """The clustering workspace of (device, K): zeroed once, reused by every call (ncn_cluster_loss
    leaves its grid-barrier words at zero).  Created on the first (eager) call, so a captured step
    reuses it.  Calls on one device are stream-ordered in this package (one training stream)."""
    key = (str(dev), K)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.zeros(int(_lib.lib().ncn_cluster_workspace_words(K)), dtype=torch.float32, device=dev)
        _WS[key] = ws
    return ws


_PLANS = {}


def kmeans_plan(dev, n_tri, K, seed=1234):
    """faiss's k-means draws for (n_tri, K, seed) (ncn_kmeans_plan_fill, built on the host once with
    std::mt19937 and kept on `dev`): subsample membership, init picks, split floats."""
    key = (str(dev), int(n_tri), int(K), int(seed))
    plan = _PLANS.get(key)
    if plan is None:
        words = int(_lib.lib().ncn_kmeans_plan_words(n_tri, K))
        host = torch.zeros(words, dtype=torch.int32)
        call("ncn_kmeans_plan_fill", n_tri, K, seed, host)
        plan = host.to(dev)
        _PLANS[key] = plan
    return plan


def cluster_launch(normals, K, niter, seed, t_sim, w, w_dev=None, step_dev=None, sched=(0.0, 1.0), photo=None):
    """The one ncn_cluster_loss launch on (T, 3) normals: allocates its outputs and fetches the
    (device, K) workspace and the (T, K, seed) plan.  w: host weights, overridden by the device
    weights w_dev; step_dev + sched = (start, grow): the weight schedule on the device; photo: the
    photometric terms for the loss total.  -> raw (N_OUT), labels (T), centroids (K, 3), dn (3, T, 3)."""
    T, dev = normals.shape[0], normals.device
    out = torch.empty(N_OUT, dtype=torch.float32, device=dev)
    labels = torch.empty(T, dtype=torch.int32, device=dev)
    cents = torch.empty(K, 3, dtype=torch.float32, device=dev)
    dn = torch.empty(3, T, 3, dtype=torch.float32, device=dev)
    call("ncn_cluster_loss", normals, T, K, niter, kmeans_plan(dev, T, K, seed), t_sim, w[0], w[1], w[2], w_dev,
         step_dev, sched[0], sched[1], photo, out, labels, cents, dn, _cluster_workspace(dev, K))
    return out, labels, cents, dn


def check_cluster_status(dev=None):
    """Raise if a clustering launch on any workspace (of `dev`, or all) hit its barrier/hand-off
    timeout (the kernel's sticky error word, ncn_cluster_status_offset): its losses and gradients
    were computed from incomplete partial sums.  One device read per workspace (host sync)."""
    for (d, K), ws in _WS.items():
        if dev is not None and d != str(dev):
            continue
        off = int(_lib.lib().ncn_cluster_status_offset(K))
        if int(ws.view(torch.int32)[off].item()) != 0:
            raise _lib.NcnError(f"ncn_cluster_loss on {d} (K={K}): a grid barrier / Lloyd hand-off timed out "
                                f"(its workgroups were not co-resident); cluster losses are invalid")


class _Normals(torch.autograd.Function):
    """hypersim_src/utils.py:504-541: n = normalize(cross(P2-P1, P3-P1)), P = rays_o + rays_d*depth."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, depth, x1, x2, x3):
        T = x1.shape[0]
        normals = torch.empty(T, 3, dtype=torch.float32, device=depth.device)
        call("ncn_normals_fwd", rays_o, rays_d, depth, x1, x2, x3, T, normals)
        ctx.save_for_backward(rays_o, rays_d, depth, x1, x2, x3)
        return normals

    @staticmethod
    def backward(ctx, dn):
        rays_o, rays_d, depth, x1, x2, x3 = ctx.saved_tensors
        ddepth = torch.zeros_like(depth)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            # pose refinement: the rays require grad (the reference's plain torch ops differentiate
            # into them; with quirk q1, rays_o := rays_d, this is how the normal terms reach the poses)
            d_o, d_d = torch.zeros_like(rays_o), torch.zeros_like(rays_d)
            if dn is not None:
                call("ncn_normals_bwd_rays", rays_o, rays_d, depth, x1, x2, x3,
                     x1.shape[0], dn.contiguous().float(), None, ddepth, d_o, d_d)
            return (d_o if ctx.needs_input_grad[0] else None, d_d if ctx.needs_input_grad[1] else None, ddepth,
                    None, None, None)
        if dn is not None:
            call("ncn_normals_bwd", rays_o, rays_d, depth, x1, x2, x3, x1.shape[0], dn.contiguous(), None, ddepth)
        return None, None, ddepth, None, None, None


def _ray_args(rays_o, rays_d, depth, x123_idx):
    """The normals nodes' tensor arguments: fp32 / int64, contiguous, on the GPU."""
    for t, n in ((rays_o, "rays_o"), (rays_d, "rays_d"), (depth, "depth")):
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
    return tuple(t.float().contiguous() for t in (rays_o, rays_d, depth)) + tuple(
        x123_idx[k].long().contiguous() for k in ("x1", "x2", "x3"))


def extract_normals_from_ray_batch(rays_o, rays_d, depth, x123_idx):
    """Drop-in for datasets/hypersim_src/utils.py:_extract_normals_from_ray_batch (fp32)."""
    return _Normals.apply(*_ray_args(rays_o, rays_d, depth, x123_idx))


class _ClusterLoss(torch.autograd.Function):
    """losses.py:420-478 on the GPU.  Returns the three weighted terms (ort, centr_dot, centr_L1)
    and, as non-differentiable extras, the labels and the k-means centroids."""

    @staticmethod
    def forward(ctx, normals, K, niter, seed, t_sim, w):
        out, labels, cents, dn = cluster_launch(normals, K, niter, seed, t_sim, *_split_weights(w))
        ctx.save_for_backward(dn)
        terms = out[4:7].clone()
        ctx.mark_non_differentiable(labels, cents, out)
        return terms, labels, cents, out

    @staticmethod
    def backward(ctx, g, _g_labels, _g_cents, _g_out):
        (dn,) = ctx.saved_tensors
        if g is None:
            return None, None, None, None, None, None
        g = g.float()
        return g[0] * dn[0] + g[1] * dn[1] + g[2] * dn[2], None, None, None, None, None


def _split_weights(w):
    """(host weights, device weights or None): w is 3 floats or a device tensor of 3 (the
    step-dependent schedule evaluated on the device)."""
    if isinstance(w, torch.Tensor):
        return (0.0, 0.0, 0.0), w.float().contiguous()
    return tuple(float(x) for x in w), None


def _weights_arg(w):
    return w if isinstance(w, torch.Tensor) else tuple(float(x) for x in w)


def cluster_losses(norm_depth, K=K_CLUSTERS, niter=K_ITERS, seed=1234, t_similar=0.99, w=(1.0, 1.0, 1.0)):
    """Weighted (ort, centr_dot, centr_L1) terms, labels (+-1..3, 0, -9 invalid), centroids, raw stats."""
    check_input(norm_depth, "norm_depth")
    return _ClusterLoss.apply(norm_depth, K, niter, seed, t_similar, _weights_arg(w))


_C = _lib.CONSTANTS  # the `terms` bits of include/ncnerf_geom.h: 1, 2, 4, 8
GEOM_DEPTH, GEOM_NORM_L1, GEOM_NORM_DOT, GEOM_REG = (_C["NCN_GEOM_DEPTH"], _C["NCN_GEOM_NORM_L1"], _C["NCN_GEOM_NORM_DOT"],
                                                     _C["NCN_GEOM_REG"])
GEOM_KEYS = ("depth", "norm_D_L1", "norm_D_dot", "reg_depth")  # the node's four terms, in its order


def geom_workspace_doubles(n_rays, n_tri):
    """ncn_geom_loss_fwd's workspace: 6 * G(max(n_rays, n_tri, 1)), G(n) = min(ceil(n / 256), 1024)."""
    return 6 * min(-(-max(n_rays, n_tri, 1) // 256), 1024)


class _GeomLoss(torch.autograd.Function):
    """losses.py:372-417 on the GPU: the depth, GT-normal L1 / dot and RegNeRF terms of `terms` in one
    forward and one backward entry point (at most two kernels each, ncnerf_geom.h).  Returns the four weighted terms after the validity
    filter (0-d, differentiable; 0 for a term that is off or filtered) and, as non-differentiable
    extras, the kernel's row (8: the terms, their raw sums) and counts (8: mask sizes, live flags).
    rays (rays_o, rays_d) or None: with them `normals` is taken as ncn_normals_fwd of (rays, depth,
    triangles) and not differentiated itself: the normal terms' gradient arrives in dL/ddepth."""

    @staticmethod
    def forward(ctx, depth, normals, depth_gt, normals_gt, x1, x2, x3, terms, w, step_dev, step, reg_start, rays):
        R, T = depth.shape[0], (0 if x1 is None else x1.shape[0])
        dev = depth.device
        ws = torch.empty(geom_workspace_doubles(R, T), dtype=torch.float64, device=dev)
        out = torch.empty(8, dtype=torch.float32, device=dev)
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        call("ncn_geom_loss_fwd", depth, depth_gt, R, normals, normals_gt, x1, x2, x3, T, terms, w[0], w[1], w[2],
             step_dev, step, reg_start, ws, ws.numel(), out, counts)
        ro, rd = rays if rays is not None else (None, None)
        ctx.save_for_backward(depth, normals, depth_gt, normals_gt, x1, x2, x3, counts, ro, rd)
        ctx.terms, ctx.w = terms, w
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(out, counts)
        return out[0], out[1], out[2], out[3], out, counts

    @staticmethod
    def backward(ctx, g_depth, g_l1, g_dot, g_reg, _g_out, _g_counts):
        depth, normals, depth_gt, normals_gt, x1, x2, x3, counts, ro, rd = ctx.saved_tensors
        gs = (g_depth, g_l1, g_dot, g_reg)
        none = (None,) * 13
        if all(g is None for g in gs):
            return none
        z = torch.zeros((), dtype=torch.float32, device=depth.device)
        up = torch.stack([z if g is None else g.float().reshape(()) for g in gs])
        ddepth = torch.empty_like(depth) if ctx.needs_input_grad[0] else None
        dn = torch.empty_like(normals) if normals is not None and ro is None and ctx.needs_input_grad[1] else None
        if ddepth is None and dn is None:
            return none
        call("ncn_geom_loss_bwd", depth, depth_gt, depth.shape[0], normals, normals_gt, x1, x2, x3,
             0 if x1 is None else x1.shape[0], ro, rd, ctx.terms, ctx.w[0], ctx.w[1], ctx.w[2], counts, up, ddepth, dn)
        return (ddepth, dn) + none[2:]


def geometry_losses(depth, x123_idx=None, depth_gt=None, normals=None, normals_gt=None, terms=0, w=(1.0, 1.0, 1.0),
                    step=0, reg_start=0, rays=None):
    """The geometry terms of `terms` (GEOM_* bits) on depth (R): depth L2 against depth_gt (R) over
    depth_gt > 0; L1 / (1 - cos) of normals (T, 3) against normals_gt[x1] over its non-zero rows,
    normals_gt (R, 3); RegNeRF over the triangles x123_idx while step > reg_start.  w: the weights of
    the first three terms; step: an int, or a device int64 scalar (read by the kernel: no host read).
    rays = (rays_o, rays_d) (R, 3): `normals` are extract_normals_from_ray_batch of these rays, the
    depth and the triangles, and the normal terms back-propagate to the depth through them inside the
    node (normals itself gets no gradient); without rays they back-propagate to `normals`.
    -> ((depth, norm_D_L1, norm_D_dot, reg_depth) 0-d tensors, row (8) f32, counts (8) int64)."""
    f = lambda t: None if t is None else t.float().contiguous()
    terms = int(terms)
    if not 0 <= terms < 16:
        raise ValueError(f"terms {terms}: a sum of GEOM_DEPTH, GEOM_NORM_L1, GEOM_NORM_DOT, GEOM_REG")
    need_norm, need_tri = terms & (GEOM_NORM_L1 | GEOM_NORM_DOT), terms & (GEOM_NORM_L1 | GEOM_NORM_DOT | GEOM_REG)
    given = [(depth, "depth")]
    given += [(depth_gt, "depth_gt")] if terms & GEOM_DEPTH else []
    given += [(normals, "normals"), (normals_gt, "normals_gt")] if need_norm else []
    for t, n in given:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
    R = depth.shape[0]
    if depth.dim() != 1:
        raise ValueError(f"depth must be (R) (got {tuple(depth.shape)})")
    x1 = x2 = x3 = None
    if need_tri:
        if x123_idx is None:
            raise ValueError("the normal and RegNeRF terms need the triangles x123_idx")
        x1, x2, x3 = (x123_idx[k].long().contiguous() for k in ("x1", "x2", "x3"))
        for x in (x1, x2, x3):
            check_input(x, "x123_idx")
        if not (x1.shape == x2.shape == x3.shape and x1.dim() == 1):
            raise ValueError("x123_idx: x1, x2 and x3 must be (T) each")
    if terms & GEOM_DEPTH:
        if depth_gt.numel() != R:
            raise ValueError(f"depth_gt must cover the {R} rays of depth (got {tuple(depth_gt.shape)})")
        depth_gt = f(depth_gt).reshape(-1)
    else:
        depth_gt = None
    if need_norm:
        if tuple(normals.shape) != (x1.shape[0], 3):
            raise ValueError(f"normals must be ({x1.shape[0]}, 3) (got {tuple(normals.shape)})")
        if tuple(normals_gt.shape) != (R, 3):
            raise ValueError(f"normals_gt must be ({R}, 3) (got {tuple(normals_gt.shape)})")
        normals, normals_gt = f(normals), f(normals_gt)
        if rays is not None:
            for t, n in zip(rays, ("rays_o", "rays_d")):
                if not isinstance(t, torch.Tensor) or not t.is_cuda:
                    raise RuntimeError(f"{n} must be a CUDA tensor")
                if tuple(t.shape) != (R, 3):
                    raise ValueError(f"{n} must be ({R}, 3) (got {tuple(t.shape)})")
            rays, normals = (f(rays[0]).detach(), f(rays[1]).detach()), normals.detach()
    else:
        normals = normals_gt = rays = None
    if isinstance(step, torch.Tensor):
        if not step.is_cuda:
            raise RuntimeError("step must be an int or a CUDA tensor")
        step_dev, step = step.to(torch.int64).reshape(()).contiguous(), 0
    else:
        step_dev, step = None, int(step)
    res = _GeomLoss.apply(f(depth), normals, depth_gt, normals_gt, x1, x2, x3, terms, tuple(float(x) for x in w),
                          step_dev, step, int(reg_start), rays)
    return res[:4], res[4], res[5]


def _no_ray_grad(rays_need_grad, who):
    """The fused loss nodes back-propagate to the depth only: refuse rays that require grad (pose
    refinement) instead of dropping their gradient."""
    if rays_need_grad:
        raise RuntimeError(f"{who} has no gradient w.r.t. rays_o / rays_d: with rays that require grad use "
                           "extract_normals_from_ray_batch + cluster_losses (NeRFMTLoss does)")


class _NormalsClusterLoss(torch.autograd.Function):
    """`_Normals` followed by `_ClusterLoss` as one node, used when the depth normals feed only the
    clustering terms (every reference config).  The backward is one `ncn_normals_bwd` launch that
    combines the three per-term normal gradients with the upstream term gradients on the device,
    so no (T,3) normal gradient is materialised and nothing is reduced on the host."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, depth, x1, x2, x3, K, niter, seed, t_sim, w):
        _no_ray_grad(ctx.needs_input_grad[0] or ctx.needs_input_grad[1], "normals_cluster_losses")
        T = x1.shape[0]
        dev = depth.device
        normals = torch.empty(T, 3, dtype=torch.float32, device=dev)
        call("ncn_normals_fwd", rays_o, rays_d, depth, x1, x2, x3, T, normals)
        out, labels, cents, dn = cluster_launch(normals, K, niter, seed, t_sim, *_split_weights(w))
        ctx.save_for_backward(rays_o, rays_d, depth, x1, x2, x3, dn)
        terms = out[4:7].clone()
        ctx.mark_non_differentiable(normals, labels, cents, out)
        return terms, normals, labels, cents, out

    @staticmethod
    def backward(ctx, g, *_unused):
        rays_o, rays_d, depth, x1, x2, x3, dn = ctx.saved_tensors
        if g is None:
            return (None,) * 11
        ddepth = torch.zeros_like(depth)
        call("ncn_normals_bwd", rays_o, rays_d, depth, x1, x2, x3, x1.shape[0], dn, g.float().contiguous(), ddepth)
        return None, None, ddepth, None, None, None, None, None, None, None, None


def normals_cluster_losses(rays_o, rays_d, depth, x123_idx, K=K_CLUSTERS, niter=K_ITERS, seed=1234, t_similar=0.99,
                           w=(1.0, 1.0, 1.0)):
    """extract_normals_from_ray_batch + cluster_losses fused: (terms, normals, labels, centroids, raw)."""
    return _NormalsClusterLoss.apply(*_ray_args(rays_o, rays_d, depth, x123_idx), K, niter, seed, t_similar,
                                     _weights_arg(w))


class _PhotoLoss(torch.autograd.Function):
    """losses.py:349-362 with the validity filter: (mean((rgb-gt)^2), w_op * mean(-o log o)) in one
    single-workgroup reduction; the backward is one elementwise launch."""

    @staticmethod
    def forward(ctx, rgb, rgb_gt, opacity, w_op):
        R = rgb.shape[0]
        loss = torch.empty(4, dtype=torch.float32, device=rgb.device)
        call("ncn_photo_loss_fwd", rgb, rgb_gt, opacity, R, w_op, loss)
        ctx.save_for_backward(rgb, rgb_gt, opacity, loss)
        ctx.w_op = w_op
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_rgb, g_op):
        rgb, rgb_gt, opacity, loss = ctx.saved_tensors
        dev = rgb.device
        g = torch.stack([torch.zeros((), device=dev) if g_rgb is None else g_rgb.float(),
                         torch.zeros((), device=dev) if g_op is None else g_op.float()])
        drgb, dop = torch.empty_like(rgb), torch.empty_like(opacity)
        call("ncn_photo_loss_bwd", rgb, rgb_gt, opacity, rgb.shape[0], ctx.w_op, loss, g, drgb, dop)
        return drgb, None, dop, None


def photo_losses(rgb, rgb_gt, opacity, w_opacity):
    """(rgb MSE, weighted opacity entropy), each 0 when non-finite (losses.py:246-262)."""
    f = lambda t: t.float().contiguous()
    check_input(rgb, "rgb")
    check_input(opacity, "opacity")
    if rgb.shape[0] != opacity.shape[0] or rgb_gt.shape != rgb.shape:
        raise ValueError("photo_losses: rgb, rgb_gt and opacity must cover the same rays")
    return _PhotoLoss.apply(f(rgb), f(rgb_gt), f(opacity), float(w_opacity))


class _NeRFLossFused(torch.autograd.Function):
    """NeRFMTLoss of the reference configuration (losses.py:169-587 with rgb + opacity +
    normal-clustering terms, `all_images_triang_patch` 8x8 patches) as ONE autograd node:
    forward = photometric reduction + normals + the clustering pipeline, whose last kernel also
    evaluates the weight schedule from the device step and the total; backward = ONE kernel
    (ncn_nerf_loss_bwd) writing dL/drgb, dL/dopacity and dL/ddepth (gathered per ray).
    Outputs: total, rgb, opacity, ort, centr_dot, centr_L1 (all differentiable, 0-d), then the
    non-differentiable labels, centroids and raw statistics."""

    @staticmethod
    def forward(ctx, rgb, opacity, depth, rays_o, rays_d, rgb_gt, x1, x2, x3, w_op, K, niter, seed, t_sim, w,
                step_dev, sched, count_job=None):
        _no_ray_grad(ctx.needs_input_grad[3] or ctx.needs_input_grad[4], "the fused NeRFMTLoss node")
        R = rgb.shape[0]
        T = x1.shape[0]
        dev = rgb.device
        photo = torch.empty(4, dtype=torch.float32, device=dev)
        normals = torch.empty(T, 3, dtype=torch.float32, device=dev)
        cj = count_job  # (custom_functions.CountJob or None)
        tot = cj.total if cj is not None else None
        call("ncn_photo_normals_count_fwd", rgb, rgb_gt, opacity, R, w_op, photo, rays_o, rays_d, depth, x1, x2, x3, T,
             normals, tot, tot.shape[0] if tot is not None else 0, cj.counter if cj else None, cj.out if cj else None,
             cj.acc if cj else None)
        out, labels, cents, dn = cluster_launch(normals, K, niter, seed, t_sim, w, None, step_dev, sched, photo)
        ctx.save_for_backward(rgb, opacity, depth, rays_o, rays_d, rgb_gt, photo, dn)
        ctx.w_op = w_op
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(labels, cents, out, normals)
        return out[10], photo[0], photo[1], out[4], out[5], out[6], labels, cents, out, normals

    @staticmethod
    def backward(ctx, g_total, g_rgb, g_op, g_ort, g_cdot, g_cl1, *_unused):
        rgb, opacity, depth, rays_o, rays_d, rgb_gt, photo, dn = ctx.saved_tensors
        dev = rgb.device
        terms = (g_rgb, g_op, g_ort, g_cdot, g_cl1)
        up_terms = None
        if any(g is not None for g in terms):  # a single term back-propagated on its own (rare)
            z = torch.zeros((), device=dev)
            up_terms = torch.stack([z if g is None else g.float().reshape(()) for g in terms]).contiguous()
        up_total = None if g_total is None else g_total.float().contiguous()
        R = rgb.shape[0]
        drgb, dop, ddepth = torch.empty_like(rgb), torch.empty_like(opacity), torch.empty_like(depth)
        call("ncn_nerf_loss_bwd", rgb, rgb_gt, opacity, R, ctx.w_op, photo, rays_o, rays_d, depth, dn, up_total,
             up_terms, drgb, dop, ddepth)
        return (drgb, dop, ddepth) + (None,) * 15


_STD_PATCH = np.arange(64).reshape(8, 8)
_STD_OFFSETS = (_STD_PATCH[1:, 1:].reshape(-1), _STD_PATCH[:-1, 1:].reshape(-1), _STD_PATCH[1:, :-1].reshape(-1))


def _standard_patch_offsets(patch_area, off):
    """True if the patch triangles are the reference's 8x8 ones (base.py:53-58), host arrays only."""
    if int(patch_area) != 64:
        return False
    for k, ref in zip(("x1", "x2", "x3"), _STD_OFFSETS):
        o = off[k]
        if isinstance(o, torch.Tensor) or not np.array_equal(np.asarray(o).reshape(-1), ref):
            return False
    return True


def _offsets_key(o):
    """Cache key of a host patch-offset array; None for tensors (indexed on the device, never read)."""
    if isinstance(o, torch.Tensor):
        return None
    return bytes(memoryview(np.ascontiguousarray(o, dtype=np.int64)))


class DistortionLoss(torch.autograd.Function):
    """losses.py:16-44: the Mip-NeRF 360 distortion loss in DVGO-v2's O(N) form
    (vren.distortion_loss_fw/bw -> ncn_distortion_loss_fw/bw).  ws, deltas, ts (S), rays_a (R,3)
    -> loss (R) by ray_idx."""

    @staticmethod
    def forward(ctx, ws, deltas, ts, rays_a):
        loss, ws_inclusive_scan, wts_inclusive_scan = vren.distortion_loss_fw(ws, deltas, ts, rays_a)
        ctx.save_for_backward(ws_inclusive_scan, wts_inclusive_scan, ws, deltas, ts, rays_a)
        return loss

    @staticmethod
    def backward(ctx, dL_dloss):
        ws_inclusive_scan, wts_inclusive_scan, ws, deltas, ts, rays_a = ctx.saved_tensors
        dL_dws = vren.distortion_loss_bw(dL_dloss.contiguous(), ws_inclusive_scan, wts_inclusive_scan, ws, deltas, ts,
                                         rays_a)
        return dL_dws, None, None, None


class NeRFMTLoss(nn.Module):
    """losses.py:169-587 (hot-path subset, see module docstring)."""

    def __init__(self, hparams_dict):
        super().__init__()
        h = hparams_dict
        self.opacity_w = h.get("loss_opacity_w", 0)
        self.distortion_w = h.get("loss_distortion_w", 0)
        self.depth_w = h.get("loss_depth_w", 0)
        self.sem_w = h.get("loss_sem_w", 0)
        self.manhattan_nerf_w = h.get("loss_manhattan_nerf_w", 0)
        self.norm_DEpth_L1_w = h.get("loss_norm_depth_L1_w", 0)
        self.norm_DEpth_dot_w = h.get("loss_norm_depth_dot_w", 0)
        self.norm_CAN_tres = h.get("loss_norm_can_tres", 0)
        self.norm_D_C_ort_dot_w = h.get("loss_norm_D_C_ort_dot_w", 0)
        self.norm_D_C_centr_dot_w = h.get("loss_norm_D_C_centr_dot_w", 0)
        self.norm_D_C_centr_L1_w = h.get("loss_norm_D_C_centr_L1_w", 0)
        self.norm_D_C_can_dot_w = h.get("loss_norm_D_C_can_dot_w", 0)
        self.norm_D_C_can_L1_w = h.get("loss_norm_D_C_can_L1_w", 0)
        self.reg_depth_w = h.get("loss_reg_depth_w", 0)
        self.ray_sampling_strategy = h.get("ray_sampling_strategy", None)
        self.random_tr_poses = h.get("random_tr_poses", False)
        self.pred_norm_depth = h.get("pred_norm_depth", False)
        self.kmeans_seed = h.get("kmeans_seed", 1234)
        for name in ("manhattan_nerf_w", "norm_D_C_can_dot_w", "norm_D_C_can_L1_w"):
            if getattr(self, name) > 0:
                raise NotImplementedError(f"loss term {name} is not part of the ported hot path (0 in all configs)")
        if self.sem_w > 0:  # losses.py:233-239
            if not h.get("pred_sem", False):
                raise NotImplementedError("loss_sem_w > 0 needs the semantic head: pred_sem in the hyper-parameters "
                                          "(the reference asserts it, losses.py:239) and NGPMT(pred_sem=True, "
                                          "n_sem_cls=K)")
            if not h.get("load_sem_gt", False) or h.get("load_sem_WF_gt", False):  # losses.py:235-236 (asserts there)
                raise ValueError("loss_sem_w > 0 needs load_sem_gt and not load_sem_WF_gt in the hyper-parameters: "
                                 "the term reads the batch's `semantics` labels")
        if self.norm_DEpth_L1_w > 0 or self.norm_DEpth_dot_w > 0:
            self.norm_GT = "normals_depth" if h.get("loss_norm_GT_depth", False) else "normals"
        start = h.get("loss_norm_can_start", 0)
        self.can_sched_start = start
        self.can_sched_end = h.get("loss_norm_can_end", -1)
        grow = h.get("loss_norm_can_grow", 1)
        self.w_sched = lambda w, step: max(0, min(w, (step - start) * (w / grow)))  # losses.py:217
        self._grow = grow
        if self.pred_norm_depth:
            assert self.ray_sampling_strategy in ["all_images_triang", "all_images_triang_val", "same_image_triang",
                                                  "all_images_triang_patch", "same_image_triang_patch"]
        self.last_cluster = None  # (labels, centroids, raw stats) of the last step, for logging/tests
        self.last_normals = None  # (fused path) the normals the clustering saw, for tests
        self._idx_cache = {}
        self._wt = {}

    @staticmethod
    def _validity(loss, dev):
        """losses.py:246-262 without host syncs: non-finite -> 0."""
        if loss.nelement() != 1:
            return torch.tensor(0.0, device=dev)
        return torch.where(torch.isfinite(loss), loss, torch.zeros_like(loss))

    @property
    def clustering(self):
        return self.norm_D_C_ort_dot_w > 0 or self.norm_D_C_centr_dot_w > 0 or self.norm_D_C_centr_L1_w > 0

    def reference_config(self, n_rays, n_opacity, patch_area, off, rays_grad):
        """Is this the reference configuration the fused node (_NeRFLossFused) serves?  The loss's own
        settings (rgb + opacity + clustering terms on patch-sampled depth normals, nothing else) plus
        the batch facts: n_rays supervised rays that are all the rendered ones (n_opacity), whole
        64-ray patches with the standard 8x8 offsets `off`, no ray gradients (pose refinement)."""
        return (not rays_grad and self.sem_w == 0 and self.clustering and self.pred_norm_depth
                and not self.random_tr_poses
                and self.opacity_w > 0 and self.distortion_w == 0
                and self.ray_sampling_strategy in ("all_images_triang_patch", "same_image_triang_patch")
                and self.depth_w == 0 and self.norm_DEpth_L1_w == 0 and self.norm_DEpth_dot_w == 0
                and self.reg_depth_w == 0 and n_rays == n_opacity and n_rays % 64 == 0 and n_rays > 0
                and _standard_patch_offsets(patch_area, off))

    def patch_triang_idx(self, seq_len, patch_s, off, dev):
        """Ray indices x1/x2/x3 of the patch triangles (losses.py:307-313); constant for a given
        (batch, patch, offsets): cached so the step issues no H2D copies."""
        key = (seq_len, int(patch_s), str(dev)) + tuple(_offsets_key(off[k]) for k in ("x1", "x2", "x3"))
        hit = None if None in key else self._idx_cache.get(key)
        if hit is None:
            pix = einops.rearrange(torch.arange(0, seq_len, device=dev), "(n s) -> n s", s=patch_s)
            hit = {k: einops.rearrange(pix[:, torch.as_tensor(off[k], device=dev)], "n s -> (n s)").contiguous()
                   for k in ("x1", "x2", "x3")}
            if None not in key:
                if len(self._idx_cache) > 16:
                    self._idx_cache.clear()
                self._idx_cache[key] = hit
        return hit

    def _geometry(self, pred_w_gt, pred_unsup, target_gt, step, shared, rays_grad):
        """losses.py:372-417: the depth, GT-normal and RegNeRF terms that are switched on, through
        `geometry_losses` (no host read).  shared: the supervised rays are the unsupervised ones
        (no random_tr_poses), so one node serves all four terms; otherwise the RegNeRF term, which
        runs on the unsupervised rays, is a node of its own.  With a host step the RegNeRF entry is
        absent until step > loss_norm_can_start, as in the reference; with a device step it is
        always there and 0 until then.  rays_grad (pose refinement): the normal terms back-propagate
        into the `_Normals` node, which reaches the rays; otherwise inside the geometry node."""
        sup = (GEOM_DEPTH if self.depth_w > 0 else 0) | (GEOM_NORM_L1 if self.norm_DEpth_L1_w > 0 else 0) | (
            GEOM_NORM_DOT if self.norm_DEpth_dot_w > 0 else 0)
        reg = GEOM_REG if self.reg_depth_w > 0 and (isinstance(step, torch.Tensor) or step > self.can_sched_start) else 0
        if sup & (GEOM_NORM_L1 | GEOM_NORM_DOT) and "norm_depth" not in pred_w_gt:
            raise ValueError("loss_norm_depth_L1_w / loss_norm_depth_dot_w need pred_norm_depth and a triangle "
                             "ray_sampling_strategy")
        if reg and "x123_idx" not in pred_unsup:
            raise ValueError("loss_reg_depth_w needs a triangle ray_sampling_strategy")
        w = (self.depth_w, self.norm_DEpth_L1_w, self.norm_DEpth_dot_w)
        jobs = [(sup | reg, pred_w_gt)] if shared else [(sup, pred_w_gt), (reg, pred_unsup)]
        loss_d = {}
        for terms, pred in jobs:
            if not terms:
                continue
            norm = terms & (GEOM_NORM_L1 | GEOM_NORM_DOT)
            vals, _row, _counts = geometry_losses(
                pred["depth"], pred.get("x123_idx"), target_gt.get("depth") if terms & GEOM_DEPTH else None,
                pred["norm_depth"] if norm else None, target_gt[self.norm_GT] if norm else None, terms, w,
                0 if step is None else step, self.can_sched_start,
                None if rays_grad or not norm else (pred["rays_o"], pred["rays_d"]))
            for bit, key, v in zip((GEOM_DEPTH, GEOM_NORM_L1, GEOM_NORM_DOT, GEOM_REG), GEOM_KEYS, vals):
                if terms & bit:
                    loss_d[key] = v
        return loss_d

    def _fused(self, pred_w_gt, target_gt, pred_unsup, kwargs):
        """The reference configuration in one autograd node (_NeRFLossFused)."""
        f = lambda t: t.float().contiguous()
        step = kwargs["global_step"]
        base = (self.norm_D_C_ort_dot_w, self.norm_D_C_centr_dot_w, self.norm_D_C_centr_L1_w)
        if isinstance(step, torch.Tensor):  # schedule evaluated on the device (graph-captured step)
            step_dev, w = step.to(torch.int64).reshape(()), base
            if not step_dev.is_contiguous():
                step_dev = step_dev.contiguous()
        else:
            if self.can_sched_end != -1 and step > self.can_sched_end:
                w = (0.0, 0.0, 0.0)
            else:
                w = tuple(self.w_sched(x, step) for x in base)
            step_dev = None
        x = pred_unsup["x123_idx"]
        for t, n in ((pred_w_gt["rgb"], "rgb"), (pred_unsup["depth"], "depth")):
            if not t.is_cuda:
                raise RuntimeError(f"{n} must be a CUDA tensor")
        total, l_rgb, l_op, ort, cdot, cl1, labels, cents, raw, normals = _NeRFLossFused.apply(
            f(pred_w_gt["rgb"]), f(pred_unsup["opacity"]), f(pred_unsup["depth"]), f(pred_unsup["rays_o"]),
            f(pred_unsup["rays_d"]), f(target_gt["rgb"]), x["x1"], x["x2"], x["x3"], float(self.opacity_w), K_CLUSTERS,
            K_ITERS, self.kmeans_seed, 1.0 - self.norm_CAN_tres, w, step_dev, (float(self.can_sched_start), float(self._grow)),
            kwargs.get("count_job"))
        self.last_cluster = (labels, cents, raw)
        self.last_normals = normals  # the patch triangles' normals (zero / invalid ones included)
        return {"rgb": l_rgb, "opacity": l_op, "norm_D_C_ort_dot": ort, "norm_D_C_centr_dot": cdot,
                "norm_D_C_centr_L1": cl1, "total": total}

    def forward(self, pred_raw, target_raw, **kwargs):
        pred_w_gt, target_gt, pred_unsup = {}, {}, {}
        gt_l = target_raw["rgb"].shape[0]
        for k in ("rgb", "depth", "normals", "normals_depth"):
            if k in target_raw:
                target_gt[k] = target_raw[k]
        # slices that cover the whole tensor are skipped: an autograd slice node would cost a
        # zero-fill + copy in the backward for nothing
        head = lambda t: t if t.shape[0] == gt_l else t[:gt_l]
        pred_w_gt["rgb"] = head(pred_raw["rgb"])
        pred_w_gt["depth"] = head(pred_raw["depth"])
        pred_w_gt["rays_o"] = head(pred_raw["rays_o"])
        pred_w_gt["rays_d"] = head(pred_raw["rays_d"])
        unsup_start = gt_l if self.random_tr_poses else 0
        tail = lambda t: t if unsup_start == 0 else t[unsup_start:]
        pred_unsup["opacity"] = pred_raw["opacity"]
        pred_unsup["depth"] = tail(pred_raw["depth"])
        pred_unsup["rays_o"] = tail(pred_raw["rays_o"])
        pred_unsup["rays_d"] = tail(pred_raw["rays_d"])
        dev = pred_raw["rgb"].device

        def get_triang_idx(seq_len):
            pix = einops.rearrange(torch.arange(0, seq_len, device=dev), "(n s) -> n s", s=3)
            return {"x1": pix[:, 0], "x2": pix[:, 1], "x3": pix[:, 2]}

        n_unsup, n_w_gt = pred_unsup["depth"].shape[0], pred_w_gt["rgb"].shape[0]
        off = None
        if self.ray_sampling_strategy in ["all_images_triang", "same_image_triang"]:
            pred_w_gt["x123_idx"] = get_triang_idx(n_w_gt)
            pred_unsup["x123_idx"] = get_triang_idx(n_unsup)
        elif self.ray_sampling_strategy in ["all_images_triang_patch", "same_image_triang_patch"]:
            off = {"x1": target_raw["x1_offsets_local"], "x2": target_raw["x2_offsets_local"],
                   "x3": target_raw["x3_offsets_local"]}
            pred_w_gt["x123_idx"] = self.patch_triang_idx(n_w_gt, target_raw["patch_area"], off, dev)
            pred_unsup["x123_idx"] = self.patch_triang_idx(n_unsup, target_raw["patch_area"], off, dev)
        clustering = self.clustering
        # pose refinement (the rays require grad): the unfused _Normals + cluster_losses branch, whose
        # backward reaches the rays; the fused nodes stop at the depth
        rays_grad = torch.is_grad_enabled() and (pred_raw["rays_o"].requires_grad or pred_raw["rays_d"].requires_grad)
        if self.reference_config(n_w_gt, pred_unsup["opacity"].shape[0], target_raw.get("patch_area", 0), off, rays_grad):
            return self._fused(pred_w_gt, target_gt, pred_unsup, dict(kwargs, count_job=pred_raw.get("_count_job")))
        job = pred_raw.get("_count_job")
        if job is not None:  # render left its sample count to the fused node, not used in this configuration
            call("ncn_count_samples", job.total, job.total.shape[0], job.counter, job.out, job.acc)
        fuse_normals = (clustering and self.pred_norm_depth and unsup_start == 0 and self.norm_DEpth_L1_w == 0
                        and self.norm_DEpth_dot_w == 0 and not rays_grad)
        if self.pred_norm_depth and not fuse_normals:
            pred_w_gt["norm_depth"] = extract_normals_from_ray_batch(pred_w_gt["rays_o"], pred_w_gt["rays_d"],
                                                                     pred_w_gt["depth"], pred_w_gt["x123_idx"])
            if unsup_start == 0:
                pred_unsup["norm_depth"] = pred_w_gt["norm_depth"]
            else:
                pred_unsup["norm_depth"] = extract_normals_from_ray_batch(pred_unsup["rays_o"], pred_unsup["rays_d"],
                                                                          pred_unsup["depth"], pred_unsup["x123_idx"])
        loss_d = {}
        if self.opacity_w > 0 and pred_w_gt["rgb"].shape[0] == pred_unsup["opacity"].shape[0]:
            loss_d["rgb"], loss_d["opacity"] = photo_losses(pred_w_gt["rgb"], target_gt["rgb"], pred_unsup["opacity"],
                                                            self.opacity_w)
        else:
            rgb_loss = ((pred_w_gt["rgb"] - target_gt["rgb"]) ** 2).mean()
            loss_d["rgb"] = self._validity(rgb_loss, dev)
        if self.opacity_w > 0 and "opacity" not in loss_d:
            o = pred_unsup["opacity"] + 1e-10
            loss_d["opacity"] = self._validity(self.opacity_w * (-o * torch.log(o)).mean(), dev)
        if self.distortion_w > 0:  # losses.py:365-369 with quirk q5: ws := ts (losses.py:290)
            ts = pred_raw["ts"].float().contiguous()
            dist = DistortionLoss.apply(ts, pred_raw["deltas"].float().contiguous(), ts, pred_raw["rays_a"].contiguous())
            loss_d["distortion"] = self._validity(self.distortion_w * dist.mean(), dev)
        step_t = isinstance(kwargs.get("global_step"), torch.Tensor)
        if step_t and self.can_sched_end != -1:
            raise NotImplementedError("a device global_step needs step-independent control flow "
                                      "(loss_norm_can_end == -1)")
        loss_d.update(self._geometry(pred_w_gt, pred_unsup, target_gt, kwargs.get("global_step"), unsup_start == 0,
                                     rays_grad))
        if clustering:
            step = kwargs["global_step"]
            if step_t or step <= self.can_sched_end or self.can_sched_end == -1:
                if step_t:  # the schedule on the device (graph-captured step): clamp((s-start)*w/grow, 0, w)
                    wt = self._wt.get(dev)
                    if wt is None:  # created once, before any capture (no H2D copy inside a graph)
                        wt = torch.tensor([self.norm_D_C_ort_dot_w, self.norm_D_C_centr_dot_w,
                                           self.norm_D_C_centr_L1_w], dtype=torch.float32, device=dev)
                        self._wt[dev] = wt
                    ramp = (step.float() - float(self.can_sched_start)) * (wt / float(self._grow))
                    w = torch.minimum(torch.clamp_min(ramp, 0.0), wt)
                else:
                    w = (self.w_sched(self.norm_D_C_ort_dot_w, step), self.w_sched(self.norm_D_C_centr_dot_w, step),
                         self.w_sched(self.norm_D_C_centr_L1_w, step))
                if fuse_normals:
                    terms, _normals, labels, cents, raw = normals_cluster_losses(
                        pred_unsup["rays_o"], pred_unsup["rays_d"], pred_unsup["depth"], pred_unsup["x123_idx"],
                        seed=self.kmeans_seed, t_similar=1.0 - self.norm_CAN_tres, w=w)
                else:
                    terms, labels, cents, raw = cluster_losses(pred_unsup["norm_depth"], seed=self.kmeans_seed,
                                                               t_similar=1.0 - self.norm_CAN_tres, w=w)
                loss_d["norm_D_C_ort_dot"] = terms[0]
                loss_d["norm_D_C_centr_dot"] = terms[1]
                loss_d["norm_D_C_centr_L1"] = terms[2]
                self.last_cluster = (labels, cents, raw)
        if self.sem_w > 0:  # losses.py:568-573
            loss_d["sem"] = self._semantic(head(pred_raw["sem"]), target_raw["semantics"])
        loss_d["total"] = sum(lo for lo in loss_d.values())
        return loss_d

    def _semantic(self, logits, labels):
        """loss_sem_w * CrossEntropyLoss(ignore_index=-1)(logits, labels - 1) (losses.py:240-242: label 0
        is void), then the validity filter; the mean as sum / max(count, 1), so an all-void batch gives
        an exact 0 with exact zero gradients instead of the 0 / 0 the filter would have to replace."""
        if not logits.is_cuda:
            raise RuntimeError("sem must be a CUDA tensor")
        t = labels.reshape(-1).long() - 1
        ce = F.cross_entropy(logits.float(), t, ignore_index=-1, reduction="sum")
        count = (t != -1).sum().clamp_min(1).to(ce.dtype)
        return self._validity(self.sem_w * (ce / count), logits.device)
