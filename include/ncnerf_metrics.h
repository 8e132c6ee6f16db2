/*
 * ncnerf_metrics.h — the validation metrics of libncnerf.so: the per-view quantities of the
 * reference's NeRFMTMetricsPerIm (metrics/metrics.py: rgb_metrics.py, depth_metrics.py,
 * normals_metrics.py) on the device.  A second header beside ncnerf.h, in the same grammar and under
 * the same rules (ncnerf.h, top): plain device pointers, `void* stream` last, nothing allocated,
 * nothing synchronised, 0 or a hipError_t returned.  THIS FILE IS PARSED by ncnerf_amd/_lib.py
 * exactly as ncnerf.h is; every entry point here returns int.
 *
 * Images are (H*W, 3) f32 pixel-major, as the renderer writes them; depth is (H*W) f32; normals are
 * (H*W, 3) f32.  Every sum is taken in a fixed order (per thread, per wave, per workgroup, then over
 * the workgroups' partial sums by one workgroup) with no float atomics: two calls on the same inputs
 * give the same bits.  Partial sums live in caller workspaces of doubles, sized below; nothing has to
 * be zeroed by the caller.
 *
 * Workspace sizes (P(n) = min(ceil(n / 256), 1024) workgroups of a streaming pass):
 *   ncn_metrics_pointwise  ws_doubles >= 6 * P(n_pix)
 *   ncn_metrics_ssim       ws_doubles >= 3 * ceil(W / 64) * ceil(H / 8)
 *   ncn_metrics_angles     ws_doubles >= 4 * P(n_pix)
 *   ncn_select_median      ws_words   >= 5120 * n_arrays
 */
#ifndef NCNERF_METRICS_H
#define NCNERF_METRICS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- pointwise errors of one view.  sums[0] = sum over the 3 n_pix components of (pred - gt)^2
 *      (each term in f32, the sum in f64); over the pixels with depth_gt > 0 (a NaN is not):
 *      sums[1] = sum (pred - gt)^2, sums[2] = sum |pred - gt|, depth_count[0] their number;
 *      range = (min, max) of rgb_gt over all components, NaN if any is NaN (torch's rule).
 *      depth_pred / depth_gt may both be NULL: sums[1..2] and the count are then 0. ---- */
int ncn_metrics_pointwise(const float* rgb_pred, const float* rgb_gt, const float* depth_pred, const float* depth_gt,
                          int64_t n_pix, double* ws, int64_t ws_doubles, double* sums, int64_t* depth_count,
                          float* range, void* stream);

/* ---- the three SSIMs of one view, one pass over LDS tiles of both images (5-pixel halo).
 *      ssim[0]: 11x11 Gaussian window (sigma 1.5), data range 1 (torchmetrics
 *      StructuralSimilarityIndexMeasure(data_range=1)); ssim[1]: the same maps with data range
 *      R = range[1] - range[0]; ssim[2]: uniform 7x7 window, sample covariance, data range R
 *      (skimage structural_similarity's defaults).  Each is the mean over the 3 channels and the
 *      pixels whose window lies inside the image.  range is read on the device.  Every window is
 *      centred on a nearby pixel before its moments are taken (variances are shift invariant), so
 *      f32 does not cancel on flat bright regions.  maps, unless NULL, is (3, H, W, 3) f32: the
 *      per-pixel value of each SSIM, written where its window lies inside the image and left
 *      untouched elsewhere.  H, W >= 11.
 *      NCN_SSIM_TAPS: the Gaussian taps g[|d|], d = 0..5, as torch computes them in f32 (arange(-5, 6),
 *      exp(-(d / 1.5)^2 / 2), divided by its sum), bit for bit (tests/test_metrics_host.py): the
 *      window is the f32 product g g^T, and its weights sum to 1 - 9.3e-8, not to 1.  Where the data
 *      range is small that excess is a visible part of sigma = E[x^2] - mu^2 (it enters as
 *      eps (mu_p - mu_t)^2 against c2), so the taps are constants here and not an expf() of the host's
 *      libm, which gives other last bits and another excess. ---- */
#define NCN_SSIM_TAPS { 0x1.10656p-2f, 0x1.b43c3ep-3f, 0x1.bff0fcp-4f, 0x1.26eb18p-5f, 0x1.f1fdf8p-8f, 0x1.0d957p-10f }
int ncn_metrics_ssim(const float* rgb_pred, const float* rgb_gt, int H, int W, const float* range, double* ws,
                     int64_t ws_doubles, float* maps, float* ssim, void* stream);

/* ---- angular errors of one view (normals_metrics.py).  Valid pixels: |gt|.sum(-1) > 0.
 *      angles is (2, n_pix) f32: the angle in degrees between pred and gt, and the smaller of it and
 *      the angle of -pred; an invalid pixel carries the marker 0xFFFFFFFF in both, a NaN angle is
 *      written as 0x7FC00000.  sums = (sum of the angles, sum of the min-angles) over the valid
 *      pixels in f64; counts = (valid pixels, valid pixels whose angle is NaN). ---- */
int ncn_metrics_angles(const float* normals_pred, const float* normals_gt, int64_t n_pix, float* angles, double* ws,
                       int64_t ws_doubles, double* sums, int64_t* counts, void* stream);

/* ---- exact selection: for each of the n_arrays rows of vals (n_arrays, capacity) f32, the k-th
 *      smallest (k = (n - 1) / 2 from 0, torch.median's lower middle) of its entries that do not
 *      carry the marker 0xFFFFFFFF, written to out[row].  n = n_dev[0] is read on the device and is
 *      the number of unmarked entries of every row; n <= 0, n > capacity, or a rank past the unmarked
 *      entries, gives NaN.
 *      Entries must be non-negative floats (their bit patterns then order as unsigned integers):
 *      three histogram passes over the 11 + 11 + 10 key bits, LDS counters flushed with integer
 *      atomics, so the result is the exact element, bit for bit. ---- */
int ncn_select_median(const float* vals, int64_t capacity, int n_arrays, const int64_t* n_dev, uint32_t* ws,
                      int64_t ws_words, float* out, void* stream);

/* ---- the view's row of 12 f32 from the device results above:
 *      psnr, ssim, ssim_n, ssim_n_sck, depth_rmse, depth_abs, depth_counted,
 *      ang_mean, ang_median, ang_mean_min, ang_median_min, norm_counted.
 *      n_rgb = 3 n_pix.  depth_count NULL, or 0 valid pixels: depth columns 0, not counted.
 *      ang_counts NULL, or 0 valid pixels: normal columns 0, not counted; one NaN angle: the four
 *      numbers are NaN and the view counts (torch's mean and median both propagate it). ---- */
int ncn_metrics_finalise(const double* pw_sums, const int64_t* depth_count, int64_t n_rgb, const float* ssim,
                         const double* ang_sums, const int64_t* ang_counts, const float* medians, float* row,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
