/*
 * ncnerf_geom.h — geometry supervision of libncnerf.so: the depth, GT-normal and RegNeRF terms of the
 * reference's NeRFMTLoss (losses.py:372-417) and the gather of their labels from device-resident
 * planes.  A third header beside ncnerf.h and ncnerf_metrics.h, in the same grammar and under the
 * same rules (ncnerf.h, top): plain device pointers, `void* stream` last, nothing allocated, nothing
 * synchronised, 0 or a hipError_t returned.  THIS FILE IS PARSED by ncnerf_amd/_lib.py exactly as
 * ncnerf.h is, into a table of its own; every entry point here returns int.
 *
 * The four terms, in the order of every 4-row below (NCN_GEOM_* are their bits in `terms`):
 *   0 depth       w_depth * mean over {i: depth_gt[i] > 0} of (depth[i] - depth_gt[i])^2
 *   1 normal L1   w_l1  * mean over the valid triangles of sum_k |n[t][k] - g[t][k]|
 *   2 normal dot  w_dot * mean over the valid triangles of 1 - cos(n[t], g[t])
 *   3 RegNeRF     mean over all triangles of (d[x1] - d[x2])^2 + (d[x1] - d[x3])^2  (no weight, as the
 *                 reference), on only while step > reg_start
 * g[t] = normals_gt[x1[t]] and a triangle is valid when |g[t]|.sum() > 0 (a NaN is not).  cos is
 * torch.nn.CosineSimilarity's: sum_k (n_k / max(|n|, 1e-8)) (g_k / max(|g|, 1e-8)), and its gradient
 * is autograd's, which differentiates the norm and not the clamp.  A term whose mask is empty, or
 * whose weighted mean is NaN or Inf, is 0 and contributes exactly zero gradient (losses.py:246-262).
 * An index of x1 / x2 / x3 outside [0, n_rays) is never dereferenced: its triangle counts as valid
 * with NaN terms, so the terms it enters are filtered.
 *
 * Every sum has a fixed order (per thread, per wave, per workgroup into the workspace, then over the
 * workgroups' partial sums by one workgroup; doubles, no float atomics): two calls on the same
 * inputs give the same bits.  Nothing has to be zeroed by the caller.
 *
 * Workspace size (G(n) = min(ceil(n / 256), 1024) workgroups):
 *   ncn_geom_loss_fwd  ws_doubles >= 6 * G(max(n_rays, n_tri, 1))
 */
#ifndef NCNERF_GEOM_H
#define NCNERF_GEOM_H
#include <stdint.h>

#define NCN_GEOM_DEPTH 1
#define NCN_GEOM_NORM_L1 2
#define NCN_GEOM_NORM_DOT 4
#define NCN_GEOM_REG 8

#ifdef __cplusplus
extern "C" {
#endif

/* ---- forward: the terms of `terms` (others: loss 0, sum 0, count 0, not live).
 *      depth (n_rays); depth_gt (n_rays), needed by the depth term; normals (n_tri, 3) and
 *      normals_gt (n_rays, 3), needed by the two normal terms; x1, x2, x3 (n_tri) int64 ray indices,
 *      needed by the normal terms (x1) and the RegNeRF term (all three).
 *      step_dev, unless NULL, is a device int64 scalar that overrides `step` (read by the kernel).
 *      out (8) f32: [0..3] the weighted terms after the validity filter, [4..7] the raw sums.
 *      counts (8) int64: [0..3] the number of mask elements of each term (triangles for 1..3),
 *      [4..7] 1 where the term is live (on, mask not empty, finite), else 0. ---- */
int ncn_geom_loss_fwd(const float* depth, const float* depth_gt, int64_t n_rays, const float* normals,
                      const float* normals_gt, const int64_t* x1, const int64_t* x2, const int64_t* x3, int64_t n_tri,
                      int terms, float w_depth, float w_l1, float w_dot, const int64_t* step_dev, int64_t step,
                      int64_t reg_start, double* ws, int64_t ws_doubles, float* out, int64_t* counts, void* stream);

/* ---- backward: out_counts = the forward's counts, upstream (4) f32 = dL / d(weighted term).
 *      ddepth (n_rays), unless NULL: every element written — the depth term's gradient by one thread
 *      per ray (a plain store, deterministic), then the triangle-to-ray scatter on top of it (float
 *      atomics): the RegNeRF term's gradient and, when rays_o / rays_d (n_rays, 3) are given, the
 *      two normal terms' gradient carried on through normals = ncn_normals_fwd(rays_o, rays_d,
 *      depth, x1, x2, x3) to the depth, as ncn_normals_bwd computes it.  A triangle that contributes
 *      nothing (masked, or no live term) is skipped there, so a filtered term leaves ddepth exactly
 *      0 even where the depth is NaN.
 *      dn (n_tri, 3), unless NULL: every element written, the gradient of the two normal terms
 *      w.r.t. `normals`, for a caller that differentiates the normals itself (ncn_normals_bwd_rays:
 *      pose refinement); rays_o and rays_d must then be NULL.  A term that is not live contributes
 *      exact zeros whatever its inputs hold. ---- */
int ncn_geom_loss_bwd(const float* depth, const float* depth_gt, int64_t n_rays, const float* normals,
                      const float* normals_gt, const int64_t* x1, const int64_t* x2, const int64_t* x3, int64_t n_tri,
                      const float* rays_o, const float* rays_d, int terms, float w_depth, float w_l1, float w_dot,
                      const int64_t* out_counts, const float* upstream, float* ddepth, float* dn, void* stream);

/* ---- label gather of a drawn batch: out_depth[r] = depth[img_idxs[r]][pix_idxs[r]], and the same
 *      for the three components of normals and normals_depth.  Planes: depth (n_images, n_pixels),
 *      normals / normals_depth (n_images, n_pixels, 3), f32.  A NULL plane is skipped (its output
 *      may be NULL too).  An index outside its range gives NaN, never an out-of-bounds read. ---- */
int ncn_batch_labels_fw(const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_rays, const float* depth,
                        const float* normals, const float* normals_depth, int n_images, int64_t n_pixels,
                        float* out_depth, float* out_normals, float* out_normals_depth, void* stream);

#ifdef __cplusplus
}
#endif
#endif
