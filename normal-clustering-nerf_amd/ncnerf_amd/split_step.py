"""The reference configuration's training step as an explicit kernel sequence with the backward
split by the gradient's source (Trainer's graph step, `split_backward`).

Same computation as render() -> NeRFMTLoss -> backward (train_nerf.py:165-358 with the loss terms
of the reference configuration, losses.py:349-362 + 420-478): the same kernels on the same inputs,
so the losses are bit-identical and the gradients agree up to f32 summation order.  What changes is
the order: the autograd backward can only start once the whole loss node (photometric + normals +
the normal clustering, ~90 us of latency-bound k-means in 16 workgroups) has finished, while the
photometric gradient does not depend on the clustering at all.  Here the photometric part is
back-propagated while the clustering runs.  The fused sequence (the default) does it on one stream,
with the rgb part of the field backward as a second role of the clustering's launch
(ncn_split_loss_fused: no queue-to-queue fork and join around the clustering):

  march -> field fwd -> composite fw
        -> [photo + normals fwd | composite bw (rgb only: dL/draws)]     one launch
        -> [cluster loss (k-means) | field MLP bwd, rgb part]             one launch
        -> loss bwd (rgb, opacity, depth) -> composite bw (all terms)
        -> field MLP bwd, sigma part -> table scatter (+ the dW slab reduction in the same launch)

The forked sequence (SplitStep(fused=False)) is the same computation on two streams, kept as the
reference of the fused one:

  main:  march -> field fwd -> composite fw -> photo+normals fwd -+-> cluster loss (k-means)
                                                                   |   -> loss bwd (depth)
  side:                                                            +-> loss bwd (rgb, opacity)
                                                                       -> composite bw (rgb)
                                                                       -> field MLP bwd, rgb part
  main (after the join): composite bw (all terms) -> field MLP bwd, sigma part -> table scatter

The rgb_net's input gradient dL/draws = w * dL/drgb needs only the photometric term, so the first
composite backward yields it exactly as the joint one would; dL/dsigma mixes all three upstream
terms and comes from the second (joint) composite backward after the clustering.
ncn_field_bwd_mlp_part's rgb pass takes the rgb_net weight gradients and the rgb part of dL/dh
(stashed in fp32); the sigma pass adds TruncExp'(h0) dL/dsigma and finishes the sigma_net and
encoding gradients.  Every per-sample value is therefore bit-identical to the autograd step's;
only the float-atomic flush order of the table gradient differs, as between any two runs.  The rgb
pass uses at most SPLIT_BLOCKS workgroups so the clustering's 16 co-resident workgroups keep CUs
of their own (an rgb-pass workgroup takes a whole CU's LDS); the sigma pass keeps only the
sigma_net's fragments and exchange tiles in LDS and runs two workgroups per CU.  Only the
fused-loss configuration takes this path (split_eligible), and only on a device that can hold the
clustering beside the rgb pass (SplitStep refuses otherwise); anything else falls back to the
autograd step."""
import ctypes

import torch

from . import _lib, vren
from ._lib import call
from .losses import K_CLUSTERS, K_ITERS, N_OUT, _STD_OFFSETS, _cluster_workspace, cluster_launch, kmeans_plan
from .ngp_mt import N_W
from .rendering import march_train_fused

SPLIT_BLOCKS = 240  # MLP-backward workgroups of each split pass at most: 256 CUs - the clustering's 16
KM_BLOCKS = 16  # the clustering kernel's co-resident workgroups (csrc/cluster_ws.h KM_BLOCKS)


def split_rgb_blocks(cus, per_cu, cap=SPLIT_BLOCKS):
    """The rgb pass's workgroups on a device of `cus` CUs where `per_cu` clustering workgroups fit
    per CU: every CU but the ceil(KM_BLOCKS / per_cu) the clustering needs, at most `cap` (240 on
    MI355X's 256 CUs).  0 when the device cannot hold the clustering at all."""
    if cus <= 0 or per_cu <= 0:
        return 0
    return max(0, min(cap, cus - -(-KM_BLOCKS // per_cu)))


def device_rgb_blocks():
    """split_rgb_blocks for the current device (ncn_cluster_coresidency with no busy CUs reports
    cus x per_cu)."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    cap = ctypes.c_int(0)
    _lib.lib().ncn_cluster_coresidency(K_CLUSTERS, 0, ctypes.byref(cap))  # rc != 0 leaves cap < 16
    return split_rgb_blocks(cus, cap.value // max(cus, 1))


def split_eligible(trainer, batch):
    """True when the step is the reference configuration the fused loss node serves
    (NeRFMTLoss.reference_config) on the static-shape white-background render."""
    L, m, kw = trainer.loss, trainer.model, trainer.render_kwargs
    R = batch["rays_o"].shape[0]
    off = {k: batch.get(k + "_offsets_local") for k in ("x1", "x2", "x3")}
    rays_grad = batch["rays_o"].requires_grad or batch["rays_d"].requires_grad  # (pose refinement: autograd)
    return (L.reference_config(batch["rgb"].shape[0], R, batch.get("patch_area", 0), off, rays_grad) and R <= 16384
            and not m.pred_norm and not m.pred_sem and getattr(m, "_aabb", None) is not None
            and kw.get("exp_step_factor", 0.0) == 0 and kw.get("anneal_strategy", "none") == "none"
            and not kw.get("random_bg", False)
            and not any(isinstance(v, torch.Tensor) for k, v in kw.items() if k != "count_acc"))


def _fused_loss(K, prec, rgb_blocks, rgb=None, rgb_gt=None, opacity=None, R=0, w_op=0.0, photo=None, rays_o=None,
                rays_d=None, depth=None, x1=None, x2=None, x3=None, T=0, normals=None, total_s=None, counter=None,
                cnt=None, acc=None, up_total=None, sigmas=None, deltas=None, rays_a=None, T_thr=0.0, draws=None,
                niter=0, plan=None, t_sim=0.0, w=(0.0, 0.0, 0.0), step_dev=None, sched=(0.0, 1.0), out=None,
                labels=None, cents=None, dn=None, workspace=None, xyzs=None, dirs=None, n=0, n_dev=None, order=None,
                packed=None, enc=None, scale=None, slab=None, dE_ws=None, lmax=None, stash=None):
    """ncn_split_loss_fused in its argument order.  With only (K, prec, rgb_blocks) nothing is
    launched: the call is the co-residency check of the fused launch for that many rgb workgroups."""
    call("ncn_split_loss_fused", rgb, rgb_gt, opacity, R, w_op, photo, rays_o, rays_d, depth, x1, x2, x3, T, normals,
         total_s, counter, cnt, acc, up_total, sigmas, deltas, rays_a, T_thr, draws, K, niter, plan, t_sim, w[0], w[1],
         w[2], None, step_dev, sched[0], sched[1], out, labels, cents, dn, workspace, xyzs, dirs, n, n_dev, order, packed,
         prec, enc, scale, rgb_blocks, slab, dE_ws, lmax, stash)


class SplitStep:
    """One training step (forward + split backward) of `trainer`'s model; run() is graph-capturable
    (no host reads).  Buffers that depend only on the batch size are allocated once."""

    def __init__(self, trainer, rgb_blocks=None, fused=True):
        """fused: the clustering and the rgb pass as two roles of one launch on one stream
        (ncn_split_loss_fused); False: the two on two streams (the forked sequence).
        rgb_blocks: the rgb pass's workgroups (one per CU), which run beside the clustering; by
        default sized from the device (device_rgb_blocks: 240 on MI355X, fewer on a smaller part).
        The clustering's workgroups meet at grid barriers, so they must all stay resident on the CUs
        the rgb pass leaves: checked here (ncn_cluster_coresidency), before the step is captured — a
        configuration where they cannot is refused (NcnError) instead of spinning into the barrier
        timeout, and Trainer then runs the autograd step.  Fused, a workgroup of either role takes a
        CU, so the 16 + rgb_blocks workgroups of the launch must fit the device by count: checked here
        as well (ncn_split_loss_fused with no rays is that check alone).  (At N > 1
        nothing else shares the step: the all-reduce of step k is stream-ordered before graph k+1,
        and RCCL's channels run beside the deferred coarse-level scatter, which leaves them 32 CUs,
        distributed.DP_SCATTER_BLOCKS.)"""
        self.tr = trainer
        self.rgb_blocks = device_rgb_blocks() if rgb_blocks is None else int(rgb_blocks)
        if self.rgb_blocks < 1:
            raise _lib.NcnError("SplitStep: the device cannot hold the clustering's workgroups beside an rgb pass")
        cap = ctypes.c_int(0)
        call("ncn_cluster_coresidency", K_CLUSTERS, self.rgb_blocks, ctypes.byref(cap))
        self.cluster_capacity = cap.value
        self.fused = bool(fused)
        if self.fused:
            _fused_loss(K_CLUSTERS, trainer.model._prec, self.rgb_blocks)

    def run(self, batch, step_dev, premarched=None):
        tr, m, L = self.tr, self.tr.model, self.tr.loss
        kw = tr.render_kwargs
        rays_o, rays_d = batch["rays_o"].contiguous().float(), batch["rays_d"].contiguous().float()
        R, dev = rays_o.shape[0], rays_o.device
        # ---- render (rendering.py:152-242 via render_rays_train's static-shape path) ----
        pm = premarched
        if pm is None:
            if not getattr(m, "_packed_fresh", False):
                m.prepare_weights()
            pm = march_train_fused(m, rays_o, rays_d, kw["near_distance"], kw["max_samples"], batch.get("march_noise"),
                                   None if "march_noise" in batch else (tr._rng_seed, step_dev))
        rays_a, xyzs, dirs, deltas, ts = pm["rays_a"], pm["xyzs"], pm["dirs"], pm["deltas"], pm["ts"]
        T_thr = kw.get("T_threshold", 1e-4)  # render_rays_train's default (rendering.py:170)
        n_dev = pm["counter"][0]
        n = xyzs.shape[0]
        sigmas, rgbs, enc, packed, order = m._field_fwd(xyzs, dirs, n_dev, 0, True)
        total_s, opacity, depth, rend, ws, rgb = vren.composite_train_multi_fw(sigmas, rgbs, deltas, ts, rays_a,
                                                                              T_thr, bg=1.0)
        # ---- NeRFMTLoss forward (_NeRFLossFused.forward) ----
        tri = L.patch_triang_idx(R, 64, dict(zip(("x1", "x2", "x3"), _STD_OFFSETS)), dev)  # (the standard 8x8 patches)
        x1, x2, x3 = tri["x1"], tri["x2"], tri["x3"]
        T = x1.shape[0]
        photo = torch.empty(4, dtype=torch.float32, device=dev)
        normals = torch.empty(T, 3, dtype=torch.float32, device=dev)
        cnt = torch.empty((), dtype=torch.int64, device=dev)
        acc = kw.get("count_acc")
        rgb_gt = batch["rgb"].contiguous().float()
        w = (L.norm_D_C_ort_dot_w, L.norm_D_C_centr_dot_w, L.norm_D_C_centr_L1_w)
        one = tr._unit(dev)
        lib = _lib.lib()
        nb = (min(self.rgb_blocks, int(lib.ncn_field_bwd_part_blocks(n, 1))),
              int(lib.ncn_field_bwd_part_blocks(n, 2)))  # (the sigma pass: two workgroups per CU)
        drgb, dop, ddepth = torch.empty_like(rgb), torch.empty_like(opacity), torch.empty_like(depth)
        slab = torch.empty(max(nb) * N_W, dtype=torch.float32, device=dev)
        dE_ws = torch.empty(int(lib.ncn_field_bwd_dE_floats(n)), dtype=torch.float32, device=dev)
        stash = torch.empty(int(lib.ncn_field_bwd_stash_floats(n)), dtype=torch.float32, device=dev)
        lmax = m._level_max()
        scale = m._bwd_loss_scale()
        g_table, g_w = m._grad_views()

        def mlp_part(part, dsig, drw):
            call("ncn_field_bwd_mlp_part", xyzs, dirs, n, n_dev, order, packed, m._prec, enc, dsig, None, drw, scale,
                 part, nb[part - 1], slab, dE_ws, lmax, stash)

        if self.fused:
            # ---- photo + normals forward and dL/draws; the clustering and the rgb pass ----
            out = torch.empty(N_OUT, dtype=torch.float32, device=dev)
            labels = torch.empty(T, dtype=torch.int32, device=dev)
            cents = torch.empty(K_CLUSTERS, 3, dtype=torch.float32, device=dev)
            dn = torch.empty(3, T, 3, dtype=torch.float32, device=dev)
            draws = torch.empty(n, 3, dtype=torch.float32, device=dev)
            _fused_loss(K_CLUSTERS, m._prec, nb[0], rgb, rgb_gt, opacity, R, L.opacity_w, photo, rays_d, rays_d, depth, x1,
                        x2, x3, T, normals, total_s, n_dev if acc is not None else None, cnt, acc, one, sigmas, deltas,
                        rays_a, float(T_thr), draws, K_ITERS, kmeans_plan(dev, T, K_CLUSTERS, L.kmeans_seed),
                        1.0 - L.norm_CAN_tres, w, step_dev, (float(L.can_sched_start), float(L._grow)), out, labels,
                        cents, dn, _cluster_workspace(dev, K_CLUSTERS), xyzs, dirs, n, n_dev, order, packed, enc, scale,
                        slab, dE_ws, lmax, stash)
            # ---- loss backward (all three gradients) -> composite (all terms) -> field MLP (sigma part) ----
            call("ncn_nerf_loss_bwd", rgb, rgb_gt, opacity, R, L.opacity_w, photo, rays_d, rays_d, depth, dn, one, None,
                 drgb, dop, ddepth)
        else:
            # (the normals use results["rays_o"] = rays_d, rendering.py:227 quirk q1)
            call("ncn_photo_normals_count_fwd", rgb, rgb_gt, opacity, R, L.opacity_w, photo, rays_d, rays_d, depth, x1,
                 x2, x3, T, normals, total_s, R, n_dev if acc is not None else None, cnt, acc)
            out, labels, cents, dn = self._forked(rgb, rgb_gt, opacity, R, photo, rays_d, depth, normals, w, step_dev,
                                                  one, drgb, dop, ddepth, sigmas, rgbs, ws, deltas, ts, rays_a, rend,
                                                  T_thr, mlp_part)
        # dL/dsigma from all three upstream terms in one expression, as the autograd step's backward
        dsig, _ = vren.composite_train_multi_bw(dop, ddepth, drgb, None, sigmas, rgbs, ws, deltas, ts, rays_a,
                                                opacity, depth, rend, T_thr, bg=1.0)
        mlp_part(2, dsig, None)
        m._scatter(xyzs, n, n_dev, order, dE_ws, lmax, g_table, wgrad=(slab, nb[1], nb[0], g_w))
        L.last_cluster = (labels, cents, out)
        L.last_normals = normals
        results = {"rays_a": rays_a, "deltas": deltas, "ts": ts, "rm_samples": n_dev, "vr_samples": cnt,
                   "opacity": opacity, "depth": depth, "ws": ws, "rgb": rgb, "rays_d": rays_d, "rays_o": rays_d,
                   "total_samples": total_s}
        loss_d = {"rgb": photo[0], "opacity": photo[1], "norm_D_C_ort_dot": out[4], "norm_D_C_centr_dot": out[5],
                  "norm_D_C_centr_L1": out[6], "total": out[10]}
        return results, loss_d

    def _forked(self, rgb, rgb_gt, opacity, R, photo, rays_d, depth, normals, w, step_dev, one, drgb, dop, ddepth,
                sigmas, rgbs, ws, deltas, ts, rays_a, rend, T_thr, mlp_part):
        """The forked sequence between the photometric forward and the joint compositor backward:
        the photometric backward on a side stream (its first launch waits for the fork; the
        clustering, issued first on this stream, takes its CUs before the rgb pass fills the rest)."""
        tr, L = self.tr, self.tr.loss
        dev = rgb.device
        cur = torch.cuda.current_stream(dev)
        side = tr._side_stream()
        side.wait_stream(cur)
        out, labels, cents, dn = cluster_launch(normals, K_CLUSTERS, K_ITERS, L.kmeans_seed, 1.0 - L.norm_CAN_tres, w,
                                                None, step_dev, (float(L.can_sched_start), float(L._grow)), photo)
        with torch.cuda.stream(side):
            # ---- photometric backward: loss -> composite -> field MLP (rgb part) ----
            call("ncn_nerf_loss_bwd", rgb, rgb_gt, opacity, R, L.opacity_w, photo, rays_d, rays_d, depth, None, one,
                 None, drgb, dop, None)
            # dL/draws = w * dL/drgb: the photometric gradient alone, bit for bit the joint backward's
            _, draws = vren.composite_train_multi_bw(dop, None, drgb, None, sigmas, rgbs, ws, deltas, ts, rays_a,
                                                     opacity, depth, rend, T_thr, bg=1.0)
            mlp_part(1, None, draws)
        # ---- clustering backward: loss (depth) -> composite (all terms) -> field MLP (sigma part) ----
        call("ncn_nerf_loss_bwd", rgb, rgb_gt, opacity, R, L.opacity_w, photo,
             rays_d, rays_d, depth, dn, one, None, None, None, ddepth)
        cur.wait_stream(side)
        return out, labels, cents, dn
