"""The validation metrics of the reference's NeRFMTMetricsPerIm (metrics/metrics.py) on the device.

  ViewMetrics.update   <- NeRFMTMetricsPerIm.update: PSNRPerImg, SSIMPerImg, SSIMPerImgNorm,
                          SSIMPerImgNormSckit (rgb_metrics.py), RMSEPerImg, AbsPerImg
                          (depth_metrics.py), AngularErrorDegPerImg(tag='depth') and, with
                          pred_norm_nn, AngularErrorDegPerImg(tag='nn') (normals_metrics.py),
                          SemanticMetrics.update with eval_sem (semantic_metrics.py)
  ViewMetrics.compute  <- NeRFMTMetricsPerIm.compute: per quantity, the sum over the views that
                          counted for it divided by their number (0 / 0 is NaN, as in the reference);
                          the semantic scores from the one confusion matrix of all views
  SemanticMetrics      <- metrics/semantic_metrics.py: update() is one streaming launch
                          (ncn_sem_confusion) that reads the renderer's `sem` slice in place, with no
                          host read per view; compute() one launch and one copy of 4 + K floats

The kernels (include/ncnerf_metrics.h, include/ncnerf_sem.h) read the renderer's (H*W, 3) pixel-major
images directly; each view leaves ONE row of 12 floats on the device (and one of 5 for the norm_nn
tag) and nothing is copied to the host before compute().  torchmetrics and scikit-image are not
needed: their definitions are restated (tests/metrics_ref.py, tests/sem_metrics_ref.py).

Not provided: LPIPS (needs VGG weights) and the wall/floor (semantics_WF) label variant.

Kept quirks of the reference: a zero predicted normal scores 90 degrees (the 1-pixel border of the
depth-image normals, pixels of depth 0); one NaN angle makes all four angular numbers of its view NaN;
a view with no valid depth / normal pixel is not counted for those quantities.  Stated deviation of
the semantic metrics: a label outside [0, K) after the shift that is not the ignore label is counted
in counts[1] and otherwise skipped (torchmetrics raises or mis-indexes on it).
"""
import torch

from ._lib import CONSTANTS, call, check_input

COLUMNS = ("psnr", "ssim", "ssim_n", "ssim_n_sck", "depth_rmse", "depth_abs", "depth_counted",
           "ang_mean", "ang_median", "ang_mean_min", "ang_median_min", "norm_counted")
NN_COLUMNS = ("ang_mean", "ang_median", "ang_mean_min", "ang_median_min", "norm_counted")  # the norm_nn tag's row
SEM_KEYS = ("miou", "miou_valid_cls", "total_acc", "cls_avg_acc")  # ncn_sem_finalise's out[0:4]
MAX_SEM_CLASSES = CONSTANTS["NCN_SEM_MAX_CLASSES"]
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


class SemanticMetrics:
    """metrics/semantic_metrics.py:SemanticMetrics(n_classes, ignore_label) on the device.

    update(pred_logits, target_labels, pred_labels=None): pred_logits (n, K) float32 CUDA with unit
    channel stride and any row stride >= K (a channel slice of a wider buffer is read in place, never
    copied); target_labels (n) of an integer dtype on CUDA, already shifted as the reference class takes
    them (ignore_label marks void); pred_labels, if given, (n) int32 CUDA: receives the argmax of every
    pixel, the void ones too (the label image the reference colour-maps).  One launch, no host read.
    conf_mat (K, K) int64 (rows the target, columns the prediction) and counts (2) int64 (pixels
    counted, labels outside [0, K) that were skipped) accumulate over the calls until reset().
    compute(): the reference's dict (miou, miou_valid_cls, total_acc, cls_avg_acc, ious) from one
    launch and ONE host copy of 4 + K floats."""

    def __init__(self, n_classes, ignore_label=-1):
        self.n_classes = _n_classes(n_classes)
        self.ignore_label = int(ignore_label)
        self._state = None

    def _buffers(self, device):
        if self._state is None or self._state.device != device:
            if self._state is not None:
                raise RuntimeError(f"SemanticMetrics: the state is on {self._state.device}, the update on {device}")
            self._state = torch.zeros(self.n_classes * self.n_classes + 2, dtype=torch.int64, device=device)
        return self._state

    @property
    def conf_mat(self):
        if self._state is None:
            raise RuntimeError("SemanticMetrics: no update yet")
        k = self.n_classes
        return self._state[:k * k].view(k, k)

    @property
    def counts(self):
        if self._state is None:
            raise RuntimeError("SemanticMetrics: no update yet")
        return self._state[self.n_classes * self.n_classes:]

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def update(self, pred_logits, target_labels, pred_labels=None, label_shift=0):
        k = self.n_classes
        logits = _logits(pred_logits, "pred_logits", k)
        n = logits.shape[0]
        labels = _labels(target_labels, "target_labels", n, logits.device)
        if pred_labels is not None:
            check_input(pred_labels, "pred_labels")
            if pred_labels.dtype != torch.int32 or pred_labels.numel() != n or pred_labels.device != logits.device:
                raise RuntimeError(f"pred_labels must be ({n}) torch.int32 on {logits.device}")
        state = self._buffers(logits.device)
        call("ncn_sem_confusion", logits, logits.stride(0) if n > 1 else k, labels, int(label_shift),
             self.ignore_label, n, k, state, state[k * k:], pred_labels)

    def finalise(self, out=None):
        """ncn_sem_finalise into out (4 + K) f32 CUDA (allocated unless given): no host copy."""
        if self._state is None:
            raise RuntimeError("SemanticMetrics: no update yet")
        if out is None:
            out = torch.empty(4 + self.n_classes, dtype=torch.float32, device=self._state.device)
        call("ncn_sem_finalise", self._state, self.n_classes, out)
        return out

    def compute(self):
        return sem_dict(self.finalise().tolist())


def sem_dict(values):
    """SemanticMetrics.compute()'s dict from the 4 + K host numbers of ncn_sem_finalise."""
    out = dict(zip(SEM_KEYS, values[:4]))
    out["ious"] = list(values[4:])
    return out


def _n_classes(k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_SEM_CLASSES:
        raise ValueError(f"n_classes = {k!r}: an int in 1..{MAX_SEM_CLASSES}")
    return k


def _logits(t, name, k):
    """(n, K) float32 CUDA, unit channel stride, rows at least K floats apart: taken in place."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be torch.float32 (got {t.dtype})")
    if t.dim() != 2 or t.shape[1] != k:
        raise ValueError(f"{name} must be (n, {k}), got {tuple(t.shape)}")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < k):
        raise RuntimeError(f"{name} must have unit channel stride and rows at least {k} floats apart "
                           f"(strides {tuple(t.stride())})")
    return t


def _labels(t, name, n, device):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise RuntimeError(f"{name} must be of an integer dtype (got {t.dtype})")
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"{name} must be ({n}), got {tuple(t.shape)}")
    if t.device != device:
        raise RuntimeError(f"{name} must be on {device}")
    return t.long().contiguous()


class ViewMetrics:
    """NeRFMTMetricsPerIm(eval_lpips=False, load_depth_gt=eval_depth, load_norm_gt=norm_gt,
    pred_norm_nn=pred_norm_nn, pred_sem and load_sem_gt=eval_sem, n_sem_cls=n_sem_cls) on the device.

    update(preds, target, h, w): preds['rgb'] (h*w,3), preds['depth'] (h*w), preds['norm_depth']
    (h*w,3); target['rgb'], target['depth'], target['normals'] likewise; float32 CUDA tensors (a CPU
    tensor raises).  Appends one device row per view, COLUMNS:
      psnr, ssim, ssim_n, ssim_n_sck, depth_rmse, depth_abs, depth_counted,
      ang_mean, ang_median, ang_mean_min, ang_median_min, norm_counted
    (*_counted is 1 or 0; the quantities of a view that is not counted are 0).
    With pred_norm_nn and norm_gt (the reference's condition) preds['norm_nn'] (h*w,3) goes through the
    same angle and median kernels and leaves a row of NN_COLUMNS (nn_rows(): (V, 5)).  With eval_sem,
    preds['sem'] (h*w, n_sem_cls) float32, read in place whatever its row stride, and target['semantics']
    (h*w) raw integer labels (0 = void) are counted into ONE confusion matrix over the views
    (self.sem: a SemanticMetrics; the reference's `target['semantics'] - 1` is the kernel's label shift).
    rows(): the (V, 12) device tensor.  compute(): ONE host copy (the rows, the nn rows and the semantic
    scores concatenated), the reference's log keys."""

    def __init__(self, eval_depth=False, norm_gt=False, pred_norm_nn=False, eval_sem=False, n_sem_cls=None):
        self.eval_depth = bool(eval_depth)
        self.norm_gt = bool(norm_gt)
        self.pred_norm_nn = bool(pred_norm_nn) and self.norm_gt  # metrics.py:37
        self.eval_sem = bool(eval_sem)
        self.sem = None
        if self.eval_sem:
            if n_sem_cls is None:
                raise ValueError("ViewMetrics(eval_sem=True) needs the class count: n_sem_cls")
            self.sem = SemanticMetrics(n_sem_cls, ignore_label=-1)  # metrics.py:46-49
        self._rows = []
        self._nn_rows = []
        self._scratch = {}

    def reset(self):
        self._rows = []
        self._nn_rows = []
        if self.sem is not None:
            self.sem.reset()

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
        if self.pred_norm_nn:
            # the same launches on the other prediction; the scratch is free again (one stream), and the
            # angular columns of a second row are the tag's row
            nn_p = _image(preds["norm_nn"].contiguous(), "preds['norm_nn']", n, 3)
            row_nn = torch.empty(len(COLUMNS), dtype=torch.float32, device=dev)
            call("ncn_metrics_angles", nn_p, nrm_t, n, s.angles, s.ang_ws, s.ang_ws.numel(), s.ang_sums, s.ang_counts)
            call("ncn_select_median", s.angles, n, 2, s.ang_counts, s.sel_ws, s.sel_ws.numel(), s.medians)
            call("ncn_metrics_finalise", s.pw_sums, None, 3 * n, s.ssim, s.ang_sums, s.ang_counts, s.medians, row_nn)
            self._nn_rows.append(row_nn[len(COLUMNS) - len(NN_COLUMNS):])
        if self.eval_sem:
            logits = preds["sem"]
            if isinstance(logits, torch.Tensor) and logits.dim() > 2:
                logits = logits.reshape(-1, logits.shape[-1])  # (a view where the strides allow it)
            self.sem.update(logits, target["semantics"].reshape(-1), label_shift=-1)  # metrics.py:86
        self._rows.append(row)
        return row

    def rows(self):
        if not self._rows:
            raise RuntimeError("ViewMetrics: no view yet")
        return torch.stack(self._rows)

    def nn_rows(self):
        """The (V, 5) device tensor of NN_COLUMNS (pred_norm_nn and norm_gt)."""
        if not self._nn_rows:
            raise RuntimeError("ViewMetrics: no norm_nn row (pred_norm_nn and norm_gt, and a view)")
        return torch.stack(self._nn_rows)

    def packed(self):
        """Everything compute() needs as ONE flat float32 device tensor: the V x 12 rows, then the
        V x 5 nn rows (pred_norm_nn), then the 4 + K semantic scores (eval_sem)."""
        parts = [self.rows().reshape(-1)]
        if self.pred_norm_nn:
            parts.append(self.nn_rows().reshape(-1))
        if self.eval_sem:
            parts.append(self.sem.finalise())
        return torch.cat(parts) if len(parts) > 1 else parts[0]

    def unpack(self, flat):
        """packed() on the host (a list) -> (rows, nn_rows or None, semantic scores or None)."""
        v, nc, nn = len(self._rows), len(COLUMNS), len(NN_COLUMNS)
        rows = [flat[i * nc:(i + 1) * nc] for i in range(v)]
        at = v * nc
        nn_rows = sem = None
        if self.pred_norm_nn:
            nn_rows = [flat[at + i * nn:at + (i + 1) * nn] for i in range(v)]
            at += v * nn
        if self.eval_sem:
            sem = flat[at:at + 4 + self.sem.n_classes]
        return rows, nn_rows, sem

    def logs(self, rows_host, nn_rows=None, sem=None):
        """The reference's log keys from the (V, 12) rows on the host (a list of lists), the (V, 5) nn
        rows and the 4 + K semantic scores where the metric has them."""
        return logs_from_rows(rows_host, self.eval_depth, self.norm_gt, nn_rows=nn_rows, sem=sem)

    def compute(self):
        return self.logs(*self.unpack(self.packed().tolist()))


def _mean_counted(rows, col, counted_col):
    n = sum(r[counted_col] for r in rows) if counted_col is not None else float(len(rows))
    total = 0.0
    for r in rows:
        if counted_col is None or r[counted_col]:
            total += r[col]
    return total / n if n else float("nan")


def logs_from_rows(rows, eval_depth, norm_gt, nn_rows=None, sem=None):
    """NeRFMTMetricsPerIm.compute() from rows of COLUMNS (host numbers).  The keys keep the
    reference's spelling ('rbg/ssim').  nn_rows: rows of NN_COLUMNS -> the norm_nn/ang_err_* keys
    (before the norm_depth ones, as the reference logs them); sem: ncn_sem_finalise's numbers -> the
    sem/* keys (the per-class ious are not logged, as in the reference)."""
    logs = {"rgb/psnr": _mean_counted(rows, 0, None), "rbg/ssim": _mean_counted(rows, 1, None),
            "rbg/ssim_n": _mean_counted(rows, 2, None), "rbg/ssim_n_sck": _mean_counted(rows, 3, None)}
    if eval_depth:
        logs["depth/rmse"] = _mean_counted(rows, 4, 6)
        logs["depth/abs"] = _mean_counted(rows, 5, 6)
    if nn_rows is not None:
        for col, name in enumerate(("mean", "median", "mean_min", "median_min")):
            logs[f"norm_nn/ang_err_{name}"] = _mean_counted(nn_rows, col, 4)
    if norm_gt:
        for name, col in (("mean", 7), ("median", 8), ("mean_min", 9), ("median_min", 10)):
            logs[f"norm_depth/ang_err_{name}"] = _mean_counted(rows, col, 11)
    if sem is not None:
        for key, value in zip(SEM_KEYS, sem):
            logs[f"sem/{key}"] = value
    return logs
