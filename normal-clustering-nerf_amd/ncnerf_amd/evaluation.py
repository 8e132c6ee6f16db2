"""Manhattan-frame evaluation of a trained field: the reference's validation path
(train_nerf.py:381-534) on the device.

  extract_normals_from_depth_batch  <- datasets/hypersim_src/utils.py:544-611 (ncn_depth_normals_image)
  normals_clustering                <- losses.py:75-166 (_normals_clustering) for any number of normals:
                                       faiss.Kmeans restated as ncn_kmeans_draws (host draws) +
                                       ncn_kmeans_train (one workgroup) + ncn_kmeans_assign (stream)
  manhattan_frame                   <- train_nerf.py:503-513 (closest +-centroids, projection on SO(3))
  evaluate_views                    <- validation_step + validation_epoch_end: render, PSNR, normals
                                       per view, ONE clustering over all views, the frame; on request
                                       val_metrics.update / compute (metrics.ViewMetrics), the norm_nn
                                       and semantic metrics included where the model has the heads

The k-means is the restatement of faiss's Clustering::train that oracle/losses_ref.py:spherical_kmeans
states (faiss itself stays parity-unpinned, as for the training loss); the normals never leave the
device (the reference copies every view's normals to the host for faiss).  The ZYX Euler-angle
differences the reference logs (train_nerf.py:521-528) follow pytorch3d's matrix_to_euler_angles
convention and are not computed here: the frame is compared by its column angles instead.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, check_input

MAX_K = 32                      # ncn_kmeans_train / ncn_kmeans_assign
MAX_POINTS_PER_CENTROID = 256   # faiss ClusteringParameters default
N_RAND = 4096                   # split_clusters' random floats handed to ncn_kmeans_train
SPLIT_SEED = 1234               # split_clusters: RandomGenerator rng(1234), whatever the k-means seed

_rand_cache = {}


def extract_normals_from_depth_batch(depth, ray_dirs_cc, poses):
    """Drop-in for _extract_normals_from_depth_batch: depth (B,H,W), ray_dirs_cc (H*W,3), poses
    (B,4,4), (B,3,4) or (B,3,3) camera-to-world -> normals (B,H,W,3) in world coordinates, zero on
    the 1-pixel border and where the pixel's depth is 0, NaN or Inf."""
    for t, n in ((depth, "depth"), (ray_dirs_cc, "ray_dirs_cc"), (poses, "poses")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
    if depth.dim() != 3:
        raise ValueError(f"depth must be (B,H,W), got {tuple(depth.shape)}")
    B, H, W = depth.shape
    if tuple(ray_dirs_cc.shape) != (H * W, 3):
        raise ValueError(f"ray_dirs_cc must be ({H * W},3), got {tuple(ray_dirs_cc.shape)}")
    if poses.dim() != 3 or poses.shape[0] != B or poses.shape[1] < 3 or poses.shape[2] < 3:
        raise ValueError(f"poses must be ({B},4,4), ({B},3,4) or ({B},3,3), got {tuple(poses.shape)}")
    depth = depth.detach().float().contiguous()
    dirs = ray_dirs_cc.detach().float().contiguous()
    rot = poses.detach()[:, :3, :3].float().contiguous()
    normals = torch.empty(B, H, W, 3, dtype=torch.float32, device=depth.device)
    call("ncn_depth_normals_image", depth, dirs, rot, B, H, W, normals)
    return normals


def kmeans_draws(nx, K, seed=1234):
    """ncn_kmeans_draws: (training set as indices into the nx points, in training order; the K
    initial picks as indices into the points; the same picks as rows of the training set), int64
    numpy arrays (host only, no GPU needed)."""
    nx, K = int(nx), int(K)
    if nx < K:
        raise ValueError(f"{nx} points for K = {K} clusters")
    sub = np.empty(min(nx, K * MAX_POINTS_PER_CENTROID), np.int64)
    init = np.empty(K, np.int64)
    rows = np.empty(K, np.int64)
    call("ncn_kmeans_draws", nx, K, int(seed) & 0xFFFFFFFF, sub.ctypes.data_as(_lib.P),
         init.ctypes.data_as(_lib.P), rows.ctypes.data_as(_lib.P))
    return sub, init, rows


def kmeans_rand_floats(seed=SPLIT_SEED, n=N_RAND):
    """ncn_kmeans_rand_floats: faiss RandomGenerator(seed).rand_float() x n, f32 numpy (host only)."""
    out = np.empty(int(n), np.float32)
    call("ncn_kmeans_rand_floats", int(seed) & 0xFFFFFFFF, int(n), out.ctypes.data_as(_lib.P))
    return out


def _rand_floats_dev(device):
    key = (device.type, device.index)
    if key not in _rand_cache:
        _rand_cache[key] = torch.from_numpy(kmeans_rand_floats()).to(device)
    return _rand_cache[key]


def spherical_kmeans(X, K, niter, seed=1234):
    """faiss.Kmeans(3, K, niter, spherical=True).train(X) + index.search(X, 1) on the VALID normals X
    (n,3) f32 CUDA, any n >= K -> (centroids (K,3) f32, assign (n) int32, counts (K) int64), all on
    the device.  One host step: the draws for the known n (no device data is read)."""
    check_input(X, "X")
    _lib.check_dtype(X, torch.float32, "X")
    if X.dim() != 2 or X.shape[1] != 3:
        raise ValueError(f"X must be (n,3), got {tuple(X.shape)}")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"K = {K}: 1..{MAX_K}")
    n, dev = X.shape[0], X.device
    if n < K:
        raise ValueError(f"{n} valid normals for K = {K} clusters")
    sub, _, rows = kmeans_draws(n, K, seed)
    train = X[torch.from_numpy(sub).to(dev)].contiguous() if n > K * MAX_POINTS_PER_CENTROID else X
    init_dev = torch.from_numpy(rows).to(dev)
    cents = torch.empty(K, 3, dtype=torch.float32, device=dev)
    call("ncn_kmeans_train", train, train.shape[0], K, int(niter), init_dev, _rand_floats_dev(dev), cents)
    assign = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(K, dtype=torch.int64, device=dev)
    call("ncn_kmeans_assign", X, n, cents, K, assign, counts)
    return cents, assign, counts


def select_clusters(centroids, counts, t_similar=0.99, merge_clusters=True, find_opposite=True):
    """The selection of losses.py:95-163 from the k-means centroids (K,3) and cluster sizes (K) on
    the host -> (table (K) int64: old cluster -> new label in {0, +-1, +-2, +-3}; (c1, c2, c3) the
    three selected clusters).  Later assignments overwrite earlier ones, as the reference's masked
    writes do, so clust_ass_new = table[clust_ass]."""
    C = np.asarray(centroids, np.float32)
    sizes = np.asarray(counts, np.int64)
    K = C.shape[0]
    sim_all = C @ C.T
    sim_abs = np.abs(sim_all)
    table = np.zeros(K, np.int64)

    def members(c_i):  # losses.py:47-54
        if merge_clusters:
            return np.nonzero(sim_all[c_i] > t_similar)[0]
        return np.array([c_i], np.int64)

    c1 = int(np.argmax(sizes))
    table[members(c1)] = 1
    crit = sim_abs[:, c1][:, None] + sim_abs[c1, :][None, :] + sim_abs
    mins, min_idxs = crit.min(axis=0), crit.argmin(axis=0)
    c2 = int(np.argmin(mins))
    c3 = int(min_idxs[c2])
    table[members(c2)] = 2
    table[members(c3)] = 3
    if find_opposite:  # losses.py:57-72, 138-163
        for lab, ci in ((-1, c1), (-2, c2), (-3, c3)):
            co = int(np.argmin(sim_all[ci]))
            if -1.0 * sim_all[ci, co] > t_similar:
                table[members(co)] = lab
    return table, (c1, c2, c3)


def valid_normals_mask(normals):
    """losses.py:427-430: all-zero, NaN or Inf rows are invalid."""
    bad = (normals.abs().sum(-1) == 0.0) | torch.isnan(normals).any(-1) | torch.isinf(normals).any(-1)
    return ~bad


def normals_clustering(normals, K=10, niter=10, t_similar=0.99, merge_clusters=True, find_opposite=True, seed=1234):
    """_normals_clustering (losses.py:75-166) for normals (..., 3) on the device, any number of them:
    -> (clust_ass_new (n) int64 in {0, +-1, +-2, +-3}, clust_ass (n) int64 k-means clusters,
    centrs_new (3,3) the selected centroids), all CUDA tensors over the n VALID rows in input order.

    Invalid rows (all-zero, NaN or Inf: the loss's rule, losses.py:427-430) are dropped first.
    Stated deviation: train_nerf.py:494 filters with `sum(-1) != 0` instead, which also drops normals
    whose components cancel and keeps NaN rows; the loss's rule is used here.  Fewer than K valid
    normals raise ValueError.  Host traffic: the valid count, and the K x 3 centroids and K counts
    for the selection."""
    if not isinstance(normals, torch.Tensor) or not normals.is_cuda:
        raise RuntimeError("normals must be a CUDA tensor")
    X = normals.detach().reshape(-1, 3).float()
    if X.shape[0] < K:
        raise ValueError(f"{X.shape[0]} normals for K = {K} clusters")
    X = X[valid_normals_mask(X)].contiguous()  # order-preserving compaction (one host read: the count)
    if X.shape[0] < K:
        raise ValueError(f"{X.shape[0]} valid normals for K = {K} clusters")
    cents, assign, counts = spherical_kmeans(X, K, niter, seed)
    cents_h = cents.cpu().numpy()
    if not np.isfinite(cents_h).all():
        raise _lib.NcnError("ncn_kmeans_train: non-finite centroids (a split walk left the random-float table)")
    table, picks = select_clusters(cents_h, counts.cpu().numpy(), t_similar, merge_clusters, find_opposite)
    clust_ass = assign.long()
    clust_ass_new = torch.from_numpy(table).to(X.device)[clust_ass]
    centrs_new = cents[torch.tensor(picks, device=X.device)]
    return clust_ass_new, clust_ass, centrs_new


def manhattan_frame(centrs_new, R_ref=None):
    """The rotation whose columns are the three selected centroids, projected onto SO(3) as
    scipy.spatial.transform.Rotation.from_matrix does (train_nerf.py:503-513) -> (R (3,3) float64
    numpy, angles).  With R_ref (3,3) each column is the one of the six +-centroids closest to
    R_ref's column (the sign and order of the clusters are arbitrary), and angles are the three
    angles in degrees between the columns of R and of R_ref; without it the centroids are taken
    in order and angles is None.  (The reference's ZYX Euler differences are not computed: module doc.)"""
    from scipy.spatial.transform import Rotation
    C = centrs_new.detach().cpu().numpy() if isinstance(centrs_new, torch.Tensor) else np.asarray(centrs_new)
    cols = C.astype(np.float64).T  # centroids as columns
    if R_ref is not None:
        Rr = R_ref.detach().cpu().numpy() if isinstance(R_ref, torch.Tensor) else np.asarray(R_ref)
        Rr = Rr.astype(np.float64)[:3, :3]
        cand = np.concatenate([cols, -cols], axis=1)  # (3,6)
        sim = cand.T @ Rr                             # (6,3): candidate j . column i of R_ref
        cols = cand[:, np.argmax(sim, axis=0)]
    R = Rotation.from_matrix(cols).as_matrix()
    if R_ref is None:
        return R, None
    cosang = np.clip((R * Rr).sum(0) / np.linalg.norm(Rr, axis=0), -1.0, 1.0)
    return R, np.degrees(np.arccos(cosang))


def evaluate_views(model, poses, ray_dirs_cc, img_wh, rgb_gt=None, K=30, niter=30, t_similar=0.99, R_ref=None,
                   depth_gt=None, normals_gt=None, metrics=False, sem_gt=None, **render_kwargs):
    """validation_step over every pose + validation_epoch_end's frame extraction.

    poses (V,3,4) or (V,4,4) camera-to-world, ray_dirs_cc (H*W,3), img_wh = (W, H), rgb_gt (V,H*W,3)
    or (V,H,W,3) or None.  Each view is rendered with render(..., test_time=True, **render_kwargs)
    (near_distance 0.01 and max_samples 1024 unless given); its PSNR = -10 log10(mean((rgb - gt)^2))
    and its depth-image normals stay on the device, and all views' normals are clustered once
    (merge_clusters=True, find_opposite=False, as train_nerf.py:495-502).
    -> {"psnr": [per view] (empty without rgb_gt), "psnr_mean", "normals" (V,H,W,3), "labels"
    (clust_ass_new of the valid normals), "centroids" (3,3), "frame" (3,3 numpy), "angles"
    (degrees to R_ref's columns, None without R_ref)}.

    With metrics=True, depth_gt (V,H*W) or (V,H,W), or normals_gt (V,H*W,3) or (V,H,W,3) in world
    coordinates, every view also goes through metrics.ViewMetrics (NeRFMTMetricsPerIm.update: the three
    SSIMs; the depth errors with depth_gt; the angular errors of the depth-image normals with
    normals_gt), which needs rgb_gt, and the result gains "metrics" (ViewMetrics.compute()'s log
    keys) and "per_view" (one {column: value} per view).  The PSNRs are then column 0 of the rows, so
    there is still one device-to-host copy outside the renderer and the clustering.

    With normals_gt and a model with the normal head (model.pred_norm: the reference's `pred_norm_nn and
    load_norm_gt`) the rendered `norm_nn` is scored too: "metrics" gains norm_nn/ang_err_* and every
    "per_view" entry the columns nn_ang_mean, nn_ang_median, nn_ang_mean_min, nn_ang_median_min,
    nn_norm_counted.  With sem_gt (V,H*W) or (V,H,W), raw integer labels with 0 = void, the rendered
    `sem` logits are counted into one confusion matrix over the views (ncn_sem_confusion reads the slice
    of the render buffer in place): "metrics" gains sem/miou, sem/miou_valid_cls, sem/total_acc,
    sem/cls_avg_acc, and the result "sem_ious" (the per-class list) and "conf_mat" (K,K int64, on the
    device).  sem_gt needs a model with the semantic head (model.pred_sem) and n_sem_cls among the
    render arguments: ValueError otherwise.  The host copy stays the one."""
    from .metrics import COLUMNS, NN_COLUMNS, ViewMetrics
    from .rendering import render
    vm = None
    if sem_gt is not None:
        if not getattr(model, "pred_sem", False):
            raise ValueError("evaluate_views: sem_gt needs a model with the semantic head (pred_sem=True)")
        if render_kwargs.get("n_sem_cls") is None:
            raise ValueError("evaluate_views: sem_gt needs n_sem_cls among the render arguments")
    if metrics or depth_gt is not None or normals_gt is not None or sem_gt is not None:
        if rgb_gt is None:
            raise ValueError("evaluate_views: the metrics need rgb_gt")
        vm = ViewMetrics(eval_depth=depth_gt is not None, norm_gt=normals_gt is not None,
                         pred_norm_nn=bool(getattr(model, "pred_norm", False)), eval_sem=sem_gt is not None,
                         n_sem_cls=render_kwargs.get("n_sem_cls"))
    W, H = int(img_wh[0]), int(img_wh[1])
    poses = poses.float()
    dirs = ray_dirs_cc.float().contiguous()
    V = poses.shape[0]
    kw = dict(near_distance=0.01, max_samples=1024)
    kw.update(render_kwargs)
    kw["test_time"] = True
    normals = torch.empty(V, H, W, 3, dtype=torch.float32, device=dirs.device)
    psnr = []
    with torch.no_grad():
        for v in range(V):
            rot = poses[v, :3, :3]
            rays_d = (dirs @ rot.T).contiguous()
            rays_o = poses[v, :3, 3].expand_as(rays_d).contiguous()
            res = render(model, rays_o, rays_d, **dict(kw))
            depth = res["depth"].reshape(1, H, W)
            normals[v] = extract_normals_from_depth_batch(depth, dirs, rot[None])[0]
            if vm is not None:
                rgb = res["rgb"].reshape(-1, 3).float().contiguous()
                preds = {"rgb": rgb, "depth": res["depth"].reshape(-1).float().contiguous(),
                         "norm_depth": normals[v].reshape(-1, 3)}
                target = {"rgb": rgb_gt[v].reshape(-1, 3).to(rgb).contiguous()}
                if depth_gt is not None:
                    target["depth"] = depth_gt[v].reshape(-1).to(rgb).contiguous()
                if normals_gt is not None:
                    target["normals"] = normals_gt[v].reshape(-1, 3).to(rgb).contiguous()
                if vm.pred_norm_nn:
                    preds["norm_nn"] = res["norm_nn"].reshape(-1, 3)
                if sem_gt is not None:
                    preds["sem"] = res["sem"]  # (a channel slice of the render buffer: read in place)
                    target["semantics"] = sem_gt[v].reshape(-1).to(rgb.device)
                vm.update(preds, target, H, W)
            elif rgb_gt is not None:
                mse = ((res["rgb"].reshape(-1, 3) - rgb_gt[v].reshape(-1, 3).to(res["rgb"])) ** 2).mean()
                psnr.append(-10.0 * torch.log10(mse))
        extra = {}
        if vm is not None:
            # the one copy: V x 12 scalars (+ V x 5 of the norm_nn tag, + the 4 + K semantic scores)
            rows, nn_rows, sem = vm.unpack(vm.packed().tolist())
            psnr = [r[0] for r in rows]
            per_view = [dict(zip(COLUMNS, r)) for r in rows]
            if nn_rows is not None:
                for d, r in zip(per_view, nn_rows):
                    d.update(zip(("nn_" + c for c in NN_COLUMNS), r))
            extra = {"metrics": vm.logs(rows, nn_rows, sem), "per_view": per_view}
            if sem is not None:
                extra["sem_ious"] = list(sem[4:])
                extra["conf_mat"] = vm.sem.conf_mat
        else:
            psnr = torch.stack(psnr).tolist() if psnr else []
        labels, _, cents = normals_clustering(normals, K=K, niter=niter, t_similar=t_similar, merge_clusters=True,
                                              find_opposite=False)
    frame, angles = manhattan_frame(cents, R_ref)
    return {"psnr": psnr, "psnr_mean": (math.fsum(psnr) / len(psnr)) if psnr else None, "normals": normals,
            "labels": labels, "centroids": cents, "frame": frame, "angles": angles, **extra}
