"""The validation metrics of the reference's NeRFMTMetricsPerIm (metrics/metrics.py) on the device.

  ViewMetrics.update   <- NeRFMTMetricsPerIm.update: PSNRPerImg, SSIMPerImg, SSIMPerImgNorm,
                          SSIMPerImgNormSckit (rgb_metrics.py), RMSEPerImg, AbsPerImg
                          (depth_metrics.py), AngularErrorDegPerImg(tag='depth') (normals_metrics.py)
  ViewMetrics.compute  <- NeRFMTMetricsPerIm.compute: per quantity, the sum over the views that
                          counted for it divided by their number (0 / 0 is NaN, as in the reference)

The kernels (include/ncnerf_metrics.h) read the renderer's (H*W, 3) pixel-major images directly; each
view leaves ONE row of 12 floats on the device and nothing is copied to the host before compute().
torchmetrics and scikit-image are not needed: their definitions are restated (DESIGN.md §3,
tests/metrics_ref.py).

Not provided: LPIPS (needs VGG weights), the semantic metrics (need the pred_sem head) and the
norm_nn angular errors (need the pred_norm head).

Kept quirks of the reference: a zero predicted normal scores 90 degrees (the 1-pixel border of the
depth-image normals, pixels of depth 0); one NaN angle makes all four angular numbers of its view NaN;
a view with no valid depth / normal pixel is not counted for those quantities.
"""
import torch

from ._lib import call, check_input

COLUMNS = ("psnr", "ssim", "ssim_n", "ssim_n_sck", "depth_rmse", "depth_abs", "depth_counted",
           "ang_mean", "ang_median", "ang_mean_min", "ang_median_min", "norm_counted")
MIN_SIDE = 11                 # the 11x11 SSIM window
# the workspace sizes include/ncnerf_metrics.h states
_STREAM_THREADS, _STREAM_MAX_BLOCKS = 256, 1024
_SSIM_TILE_W, _SSIM_TILE_H = 64, 8
SELECT_WORDS = 5120


def _stream_blocks(n):
    return min(-(-n // _STREAM_THREADS), _STREAM_MAX_BLOCKS)


def _image(t, name, n_pix, channels):
    check_input(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be torch.float32 (got {t.dtype})")
    if t.numel() != n_pix * channels:
        raise ValueError(f"{name} must hold {n_pix} x {channels} values, got {tuple(t.shape)}")
    return t


class _Scratch:
    """Everything one view's launches write besides the row, allocated once per image size."""

    def __init__(self, h, w, device, normals=True):
        n = h * w
        f64 = dict(dtype=torch.float64, device=device)
        self.pw_ws = torch.empty(6 * _stream_blocks(n), **f64)
        self.ssim_ws = torch.empty(3 * (-(-w // _SSIM_TILE_W)) * (-(-h // _SSIM_TILE_H)), **f64)
        self.pw_sums = torch.empty(3, **f64)
        self.depth_count = torch.empty(1, dtype=torch.int64, device=device)
        self.range = torch.empty(2, dtype=torch.float32, device=device)
        self.ssim = torch.empty(3, dtype=torch.float32, device=device)
        if not normals:
            return
        self.ang_ws = torch.empty(4 * _stream_blocks(n), **f64)
        self.angles = torch.empty(2, n, dtype=torch.float32, device=device)
        self.ang_sums = torch.empty(2, **f64)
        self.ang_counts = torch.empty(2, dtype=torch.int64, device=device)
        self.sel_ws = torch.empty(2 * SELECT_WORDS, dtype=torch.int32, device=device)
        self.medians = torch.empty(2, dtype=torch.float32, device=device)


def ssim_view(rgb_pred, rgb_gt, h, w, maps=False):
    """The three SSIMs of one view -> (ssim (3) f32 CUDA: ssim, ssim_n, ssim_n_sck; maps (3,h,w,3) or
    None).  maps are NaN where a window does not lie inside the image."""
    h, w = int(h), int(w)
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError(f"SSIM's 11x11 window needs an image of at least 11x11, got {h}x{w}")
    n = h * w
    _image(rgb_pred, "rgb_pred", n, 3), _image(rgb_gt, "rgb_gt", n, 3)
    s = _Scratch(h, w, rgb_pred.device, normals=False)
    call("ncn_metrics_pointwise", rgb_pred, rgb_gt, None, None, n, s.pw_ws, s.pw_ws.numel(), s.pw_sums,
         s.depth_count, s.range)
    out_maps = torch.full((3, h, w, 3), float("nan"), dtype=torch.float32, device=rgb_pred.device) if maps else None
    call("ncn_metrics_ssim", rgb_pred, rgb_gt, h, w, s.range, s.ssim_ws, s.ssim_ws.numel(), out_maps, s.ssim)
    return s.ssim, out_maps


def select_median(vals, n_dev):
    """ncn_select_median: vals (A, capacity) or (capacity) f32 CUDA of non-negative floats, entries
    with the bit pattern 0xFFFFFFFF skipped; n_dev (1) int64 CUDA, the number of unmarked entries of
    every row -> (A) f32 CUDA, each row's element of rank (n - 1) // 2 (torch.median's)."""
    check_input(vals, "vals"), check_input(n_dev, "n_dev")
    if vals.dtype != torch.float32 or n_dev.dtype != torch.int64:
        raise RuntimeError("vals must be float32 and n_dev int64")
    v = vals.reshape(1, -1) if vals.dim() == 1 else vals
    a, cap = v.shape
    ws = torch.empty(a * SELECT_WORDS, dtype=torch.int32, device=v.device)
    out = torch.empty(a, dtype=torch.float32, device=v.device)
    call("ncn_select_median", v, cap, a, n_dev, ws, ws.numel(), out)
    return out


class ViewMetrics:
    """NeRFMTMetricsPerIm(eval_lpips=False, load_depth_gt=eval_depth, load_norm_gt=norm_gt,
    pred_norm_nn=False, pred_sem=False) on the device.

    update(preds, target, h, w): preds['rgb'] (h*w,3), preds['depth'] (h*w), preds['norm_depth']
    (h*w,3); target['rgb'], target['depth'], target['normals'] likewise; float32 CUDA tensors (a CPU
    tensor raises).  Appends one device row per view, COLUMNS:
      psnr, ssim, ssim_n, ssim_n_sck, depth_rmse, depth_abs, depth_counted,
      ang_mean, ang_median, ang_mean_min, ang_median_min, norm_counted
    (*_counted is 1 or 0; the quantities of a view that is not counted are 0).
    rows(): the (V, 12) device tensor.  compute(): ONE host copy, the reference's log keys."""

    def __init__(self, eval_depth=False, norm_gt=False):
        self.eval_depth = bool(eval_depth)
        self.norm_gt = bool(norm_gt)
        self._rows = []
        self._scratch = {}

    def reset(self):
        self._rows = []

    def update(self, preds, target, h, w):
        h, w = int(h), int(w)
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError(f"SSIM's 11x11 window needs an image of at least 11x11, got {h}x{w}")
        n = h * w
        rgb_p, rgb_t = _image(preds["rgb"], "preds['rgb']", n, 3), _image(target["rgb"], "target['rgb']", n, 3)
        dev = rgb_p.device
        dep_p = dep_t = None
        if self.eval_depth:
            dep_p = _image(preds["depth"], "preds['depth']", n, 1)
            dep_t = _image(target["depth"], "target['depth']", n, 1)
        key = (h, w, dev)
        s = self._scratch.get(key)
        if s is None:
            s = self._scratch[key] = _Scratch(h, w, dev, normals=self.norm_gt)
        row = torch.empty(len(COLUMNS), dtype=torch.float32, device=dev)
        call("ncn_metrics_pointwise", rgb_p, rgb_t, dep_p, dep_t, n, s.pw_ws, s.pw_ws.numel(), s.pw_sums,
             s.depth_count, s.range)
        call("ncn_metrics_ssim", rgb_p, rgb_t, h, w, s.range, s.ssim_ws, s.ssim_ws.numel(), None, s.ssim)
        if self.norm_gt:
            nrm_p = _image(preds["norm_depth"], "preds['norm_depth']", n, 3)
            nrm_t = _image(target["normals"], "target['normals']", n, 3)
            call("ncn_metrics_angles", nrm_p, nrm_t, n, s.angles, s.ang_ws, s.ang_ws.numel(), s.ang_sums, s.ang_counts)
            call("ncn_select_median", s.angles, n, 2, s.ang_counts, s.sel_ws, s.sel_ws.numel(), s.medians)
        call("ncn_metrics_finalise", s.pw_sums, s.depth_count if self.eval_depth else None, 3 * n, s.ssim,
             s.ang_sums if self.norm_gt else None, s.ang_counts if self.norm_gt else None,
             s.medians if self.norm_gt else None, row)
        self._rows.append(row)
        return row

    def rows(self):
        if not self._rows:
            raise RuntimeError("ViewMetrics: no view yet")
        return torch.stack(self._rows)

    def logs(self, rows_host):
        """The reference's log keys from the (V, 12) rows on the host (a list of lists)."""
        return logs_from_rows(rows_host, self.eval_depth, self.norm_gt)

    def compute(self):
        return self.logs(self.rows().tolist())


def _mean_counted(rows, col, counted_col):
    n = sum(r[counted_col] for r in rows) if counted_col is not None else float(len(rows))
    total = 0.0
    for r in rows:
        if counted_col is None or r[counted_col]:
            total += r[col]
    return total / n if n else float("nan")


def logs_from_rows(rows, eval_depth, norm_gt):
    """NeRFMTMetricsPerIm.compute() from rows of COLUMNS (host numbers).  The keys keep the
    reference's spelling ('rbg/ssim')."""
    logs = {"rgb/psnr": _mean_counted(rows, 0, None), "rbg/ssim": _mean_counted(rows, 1, None),
            "rbg/ssim_n": _mean_counted(rows, 2, None), "rbg/ssim_n_sck": _mean_counted(rows, 3, None)}
    if eval_depth:
        logs["depth/rmse"] = _mean_counted(rows, 4, 6)
        logs["depth/abs"] = _mean_counted(rows, 5, 6)
    if norm_gt:
        for name, col in (("mean", 7), ("median", 8), ("mean_min", 9), ("median_min", 10)):
            logs[f"norm_depth/ang_err_{name}"] = _mean_counted(rows, col, 11)
    return logs
