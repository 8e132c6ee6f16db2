// Geometry supervision for gfx950: the depth, GT-normal and RegNeRF terms of the reference's
// NeRFMTLoss (losses.py:372-417) with its validity filter (:246-262), and the gather of their labels
// from device-resident planes — behind the C ABI of include/ncnerf_geom.h.
//  * ncn_geom_loss_fwd    one streaming pass over rays and triangles for every term that is on, its
//                         workgroups' partial sums into the workspace, then one workgroup (the
//                         fixed-order reduction of workgroup.h: doubles, no float atomics)
//  * ncn_geom_loss_bwd    dL/ddepth (one thread per ray, plain stores) and dL/dnormals (one thread
//                         per triangle) in one pass; the triangle-to-ray scatter on top: the RegNeRF
//                         term and, given the rays, the normal terms through loss_normals.h's
//                         tri_depth_grads
//  * ncn_batch_labels_fw  labels[r] = plane[img_idxs[r]][pix_idxs[r]] beside ncn_batch_rays_fw
//  * ncn_batch_semantics_fw  the same gather of an integer label plane (include/ncnerf_sem.h)
// Nothing here reads the host but its arguments, allocates or synchronises: all of them can be nodes of
// a captured step.  The per-element terms are f32, operation for operation as torch evaluates the
// reference's expressions (no contraction into fma).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include "loss_normals.h"
#include "workgroup.h"
#include "../../include/ncnerf_geom.h"
#include "../../include/ncnerf_sem.h"

namespace ncn {

constexpr int GM_THREADS = 256;
constexpr int GM_MAX_BLOCKS = 1024;  // G(n) of ncnerf_geom.h
constexpr int GM_SUMS = 6;           // depth sq, depth count, L1, dot, valid triangles, RegNeRF
constexpr float GM_COS_EPS = 1e-8f;  // torch.nn.CosineSimilarity's eps

static inline int geom_blocks(int64_t n) {
    return (int)std::min<int64_t>(cdiv(std::max<int64_t>(n, 1), GM_THREADS), GM_MAX_BLOCKS);
}

__device__ __forceinline__ bool in_range(int64_t i, int64_t n) { return i >= 0 && i < n; }
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

// 1 - cos(n, g) as torch.nn.CosineSimilarity(dim=-1) evaluates it in f32: both vectors divided by
// their norms clamped to eps, the three products summed left to right.
__device__ __forceinline__ float one_minus_cos(const float n[3], const float g[3]) {
    const float nn = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), GM_COS_EPS);
    const float gn = fmaxf(sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), GM_COS_EPS);
    return 1.0f - ((n[0] / nn) * (g[0] / gn) + (n[1] / nn) * (g[1] / gn) + (n[2] / nn) * (g[2] / gn));
}

// d cos / d n as autograd gives it: the clamp is applied outside the graph, so the quotient n / N is
// differentiated with N = max(|n|, eps) as its value and d|n| = n / |n| (0 at n = 0) as its derivative.
__device__ __forceinline__ void dcos_dn(const float n[3], const float g[3], float dc[3]) {
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const float N = fmaxf(len, GM_COS_EPS);
    const float gn = fmaxf(sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), GM_COS_EPS);
    const float gh[3] = {g[0] / gn, g[1] / gn, g[2] / gn};
    const float ng = n[0] * gh[0] + n[1] * gh[1] + n[2] * gh[2];
    const float back = len > 0.0f ? ng / (N * N * len) : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) dc[k] = gh[k] / N - back * n[k];
}

// ---- forward ----
// Grid-stride over the rays (depth term) and the triangles (normal and RegNeRF terms).
// partials[b] = the GM_SUMS sums of workgroup b.
__global__ __launch_bounds__(GM_THREADS) void geom_fwd_kernel(
    const float* __restrict__ depth, const float* __restrict__ depth_gt, int64_t R, const float* __restrict__ normals,
    const float* __restrict__ normals_gt, const int64_t* __restrict__ x1, const int64_t* __restrict__ x2,
    const int64_t* __restrict__ x3, int64_t T, int terms, const int64_t* __restrict__ step_dev, int64_t step_host,
    int64_t reg_start, double* __restrict__ partials) {
    __shared__ double red[GM_THREADS / WAVE][GM_SUMS];
    double s[GM_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const float nan = __builtin_nanf("");
    const bool norm_on = (terms & (NCN_GEOM_NORM_L1 | NCN_GEOM_NORM_DOT)) != 0;
    const bool reg_on = (terms & NCN_GEOM_REG) != 0 && (step_dev ? *step_dev : step_host) > reg_start;
    const int64_t stride = (int64_t)gridDim.x * GM_THREADS;
    const int64_t first = (int64_t)blockIdx.x * GM_THREADS + threadIdx.x;
    if (terms & NCN_GEOM_DEPTH) {
        for (int64_t i = first; i < R; i += stride) {
            const float t = depth_gt[i];
            if (t > 0.0f) {
                const float d = depth[i] - t;
                s[0] += (double)(d * d);
                s[1] += 1.0;
            }
        }
    }
    if (norm_on || reg_on) {
        for (int64_t t = first; t < T; t += stride) {
            const int64_t i1 = x1[t];
            const bool ok1 = in_range(i1, R);
            if (norm_on) {
                if (!ok1) {
                    s[2] += (double)nan;
                    s[3] += (double)nan;
                    s[4] += 1.0;
                } else {
                    const float g[3] = {normals_gt[3 * i1], normals_gt[3 * i1 + 1], normals_gt[3 * i1 + 2]};
                    if (fabsf(g[0]) + fabsf(g[1]) + fabsf(g[2]) > 0.0f) {
                        const float n[3] = {normals[3 * t], normals[3 * t + 1], normals[3 * t + 2]};
                        if (terms & NCN_GEOM_NORM_L1)
                            s[2] += (double)(fabsf(n[0] - g[0]) + fabsf(n[1] - g[1]) + fabsf(n[2] - g[2]));
                        if (terms & NCN_GEOM_NORM_DOT) s[3] += (double)one_minus_cos(n, g);
                        s[4] += 1.0;
                    }
                }
            }
            if (reg_on) {
                const int64_t i2 = x2[t], i3 = x3[t];
                if (ok1 && in_range(i2, R) && in_range(i3, R)) {
                    const float d1 = depth[i1], a = d1 - depth[i2], b = d1 - depth[i3];
                    s[5] += (double)(a * a + b * b);
                } else {
                    s[5] += (double)nan;
                }
            }
        }
    }
    block_sum<GM_SUMS, GM_THREADS>(s, red);
    if (threadIdx.x == 0) {
        double* o = partials + GM_SUMS * (int64_t)blockIdx.x;
#pragma unroll
        for (int k = 0; k < GM_SUMS; k++) o[k] = s[k];
    }
}

// One term of the row: w * mean in f32 (as torch multiplies the f32 mean), filtered.
__device__ __forceinline__ void geom_term(bool on, double sum, double count, float w, int k, float* __restrict__ out,
                                          int64_t* __restrict__ counts) {
    float loss = 0.0f;
    bool live = false;
    if (on && count > 0.0) {
        loss = w * (float)(sum / count);
        live = finite_f(loss);
    }
    out[k] = live ? loss : 0.0f;
    out[4 + k] = on ? (float)sum : 0.0f;
    counts[k] = on ? (int64_t)count : 0;
    counts[4 + k] = live ? 1 : 0;
}

__global__ __launch_bounds__(GM_THREADS) void geom_fwd_reduce_kernel(
    const double* __restrict__ partials, int nb, int64_t T, int terms, float w_depth, float w_l1, float w_dot,
    const int64_t* __restrict__ step_dev, int64_t step_host, int64_t reg_start, float* __restrict__ out,
    int64_t* __restrict__ counts) {
    __shared__ double red[GM_THREADS / WAVE][GM_SUMS];
    double s[GM_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += GM_THREADS) {
        const double* p = partials + GM_SUMS * (int64_t)b;
#pragma unroll
        for (int k = 0; k < GM_SUMS; k++) s[k] += p[k];
    }
    block_sum<GM_SUMS, GM_THREADS>(s, red);
    if (threadIdx.x != 0) return;
    const bool reg_on = (terms & NCN_GEOM_REG) != 0 && (step_dev ? *step_dev : step_host) > reg_start;
    geom_term((terms & NCN_GEOM_DEPTH) != 0, s[0], s[1], w_depth, 0, out, counts);
    geom_term((terms & NCN_GEOM_NORM_L1) != 0, s[2], s[4], w_l1, 1, out, counts);
    geom_term((terms & NCN_GEOM_NORM_DOT) != 0, s[3], s[4], w_dot, 2, out, counts);
    geom_term(reg_on, s[5], (double)T, 1.0f, 3, out, counts);
}

// ---- backward ----
// dL / d normals[t] of the live normal terms into g3; false (g3 untouched) where the triangle
// contributes nothing: no live term, an index out of range, a masked row.
__device__ __forceinline__ bool normal_terms_grad(const float* __restrict__ normals,
                                                  const float* __restrict__ normals_gt,
                                                  const int64_t* __restrict__ x1, int64_t R, int64_t t, int terms,
                                                  float w_l1, float w_dot, const int64_t* __restrict__ oc,
                                                  const float* __restrict__ up, float g3[3]) {
    const bool l1 = (terms & NCN_GEOM_NORM_L1) && oc[5] != 0, dot = (terms & NCN_GEOM_NORM_DOT) && oc[6] != 0;
    if (!l1 && !dot) return false;
    const int64_t i1 = x1[t];
    if (!in_range(i1, R)) return false;
    const float g[3] = {normals_gt[3 * i1], normals_gt[3 * i1 + 1], normals_gt[3 * i1 + 2]};
    if (!(fabsf(g[0]) + fabsf(g[1]) + fabsf(g[2]) > 0.0f)) return false;
    const float n[3] = {normals[3 * t], normals[3 * t + 1], normals[3 * t + 2]};
    g3[0] = g3[1] = g3[2] = 0.0f;
    if (l1) {
        const float c = up[1] * w_l1 / (float)oc[1];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float d = n[k] - g[k];
            g3[k] = d > 0.0f ? c : (d < 0.0f ? -c : 0.0f);
        }
    }
    if (dot) {
        const float c = up[2] * w_dot / (float)oc[2];
        float dc[3];
        dcos_dn(n, g, dc);
#pragma unroll
        for (int k = 0; k < 3; k++) g3[k] -= c * dc[k];
    }
    return true;
}

// Thread i < R writes ddepth[i] (the depth term, or 0); thread t < T writes dn[t] (the normal terms,
// or 0).  Every value of a term that is not live is a literal 0: nothing is multiplied into it.
__global__ __launch_bounds__(GM_THREADS) void geom_bwd_kernel(
    const float* __restrict__ depth, const float* __restrict__ depth_gt, int64_t R, const float* __restrict__ normals,
    const float* __restrict__ normals_gt, const int64_t* __restrict__ x1, int64_t T, int terms, float w_depth,
    float w_l1, float w_dot, const int64_t* __restrict__ oc, const float* __restrict__ up,
    float* __restrict__ ddepth, float* __restrict__ dn) {
    const int64_t i = (int64_t)blockIdx.x * GM_THREADS + threadIdx.x;
    if (ddepth != nullptr && i < R) {
        float g = 0.0f;
        if ((terms & NCN_GEOM_DEPTH) && oc[4] != 0) {
            const float t = depth_gt[i];
            if (t > 0.0f) g = (up[0] * w_depth / (float)oc[0]) * (2.0f * (depth[i] - t));
        }
        ddepth[i] = g;
    }
    if (dn != nullptr && i < T) {
        float g3[3] = {0.0f, 0.0f, 0.0f};
        normal_terms_grad(normals, normals_gt, x1, R, i, terms, w_l1, w_dot, oc, up, g3);
#pragma unroll
        for (int k = 0; k < 3; k++) dn[3 * i + k] = g3[k];
    }
}

// What the triangles scatter to their rays, on top of what geom_bwd_kernel stored (stream order): the
// RegNeRF term's gradient and, when the rays are given, the normal terms' gradient carried through
// the triangle's normal (tri_depth_grads, the body of normals_bwd_kernel).  A triangle that
// contributes nothing is skipped, so no 0 * NaN of its geometry reaches ddepth.  A ray is a corner of
// several triangles: float atomics, as normals_bwd_kernel.
__global__ __launch_bounds__(GM_THREADS) void geom_bwd_scatter_kernel(
    const float* __restrict__ depth, int64_t R, const float* __restrict__ normals, const float* __restrict__ normals_gt,
    const int64_t* __restrict__ x1, const int64_t* __restrict__ x2, const int64_t* __restrict__ x3, int64_t T,
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, int terms, float w_l1, float w_dot,
    const int64_t* __restrict__ oc, const float* __restrict__ up, float* __restrict__ ddepth) {
    const int64_t t = (int64_t)blockIdx.x * GM_THREADS + threadIdx.x;
    if (t >= T) return;
    const bool reg = (terms & NCN_GEOM_REG) && oc[7] != 0;
    float g3[3];
    const bool nrm = rays_o != nullptr && normal_terms_grad(normals, normals_gt, x1, R, t, terms, w_l1, w_dot, oc, up, g3);
    if (!reg && !nrm) return;
    const int64_t i1 = x1[t], i2 = x2[t], i3 = x3[t];
    if (!in_range(i1, R) || !in_range(i2, R) || !in_range(i3, R)) return;  // (a live term has none)
    float g1 = 0.0f, g2 = 0.0f, g3d = 0.0f;
    if (nrm) tri_depth_grads(rays_o, rays_d, depth, i1, i2, i3, g3, g1, g2, g3d);
    if (reg) {
        const float d1 = depth[i1], a = d1 - depth[i2], b = d1 - depth[i3];
        const float c = up[3] * 2.0f / (float)T;
        g1 += c * (a + b);
        g2 -= c * a;
        g3d -= c * b;
    }
    atomicAdd(ddepth + i1, g1);
    atomicAdd(ddepth + i2, g2);
    atomicAdd(ddepth + i3, g3d);
}

// ---- labels ----
__global__ __launch_bounds__(GM_THREADS) void batch_labels_fw_kernel(
    const int64_t* __restrict__ img_idxs, const int64_t* __restrict__ pix_idxs, int64_t R,
    const float* __restrict__ depth, const float* __restrict__ normals, const float* __restrict__ normals_depth,
    int n_images, int64_t HW, float* __restrict__ out_depth, float* __restrict__ out_normals,
    float* __restrict__ out_normals_depth) {
    const int64_t r = (int64_t)blockIdx.x * GM_THREADS + threadIdx.x;
    if (r >= R) return;
    const int64_t im = img_idxs[r], px = pix_idxs[r];
    const bool ok = im >= 0 && im < n_images && px >= 0 && px < HW;
    const float nan = __builtin_nanf("");
    const int64_t at = ok ? im * HW + px : 0;
    if (depth != nullptr) out_depth[r] = ok ? depth[at] : nan;
    if (normals != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; k++) out_normals[3 * r + k] = ok ? normals[3 * at + k] : nan;
    }
    if (normals_depth != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; k++) out_normals_depth[3 * r + k] = ok ? normals_depth[3 * at + k] : nan;
    }
}

// the integer plane (uint8, int32 or int64 labels): 0, void, where an index is out of range
__global__ __launch_bounds__(GM_THREADS) void batch_semantics_fw_kernel(
    const int64_t* __restrict__ img_idxs, const int64_t* __restrict__ pix_idxs, int64_t R,
    const void* __restrict__ plane, int plane_bytes, int n_images, int64_t HW, int64_t* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * GM_THREADS + threadIdx.x;
    if (r >= R) return;
    const int64_t im = img_idxs[r], px = pix_idxs[r];
    int64_t v = 0;
    if (im >= 0 && im < n_images && px >= 0 && px < HW) {
        const int64_t at = im * HW + px;
        v = plane_bytes == 1   ? (int64_t) static_cast<const uint8_t*>(plane)[at]
            : plane_bytes == 4 ? (int64_t) static_cast<const int32_t*>(plane)[at]
                               : static_cast<const int64_t*>(plane)[at];
    }
    out[r] = v;
}

}  // namespace ncn

using namespace ncn;

// What the terms of `terms` read (shared by the forward and the backward).
#define GEOM_REQUIRE_INPUTS(who)                                                                                     \
    do {                                                                                                             \
        NCN_REQUIRE(n_rays >= 0 && n_tri >= 0 && terms >= 0 && terms < 16, hipErrorInvalidValue,                     \
                    who ": bad arguments (n_rays = %lld, n_tri = %lld, terms = %d)", (long long)n_rays,              \
                    (long long)n_tri, terms);                                                                        \
        NCN_REQUIRE(!(terms & NCN_GEOM_DEPTH) || n_rays == 0 || (depth != nullptr && depth_gt != nullptr),           \
                    hipErrorInvalidValue, who ": the depth term needs depth and depth_gt");                          \
        NCN_REQUIRE(!(terms & (NCN_GEOM_NORM_L1 | NCN_GEOM_NORM_DOT)) || n_tri == 0 ||                               \
                        (normals != nullptr && normals_gt != nullptr && x1 != nullptr),                              \
                    hipErrorInvalidValue, who ": the normal terms need normals, normals_gt and x1");                 \
        NCN_REQUIRE(!(terms & NCN_GEOM_REG) || n_tri == 0 ||                                                         \
                        (depth != nullptr && x1 != nullptr && x2 != nullptr && x3 != nullptr),                       \
                    hipErrorInvalidValue, who ": the RegNeRF term needs depth, x1, x2 and x3");                      \
    } while (0)

extern "C" {

int ncn_geom_loss_fwd(const float* depth, const float* depth_gt, int64_t n_rays, const float* normals,
                      const float* normals_gt, const int64_t* x1, const int64_t* x2, const int64_t* x3, int64_t n_tri,
                      int terms, float w_depth, float w_l1, float w_dot, const int64_t* step_dev, int64_t step,
                      int64_t reg_start, double* ws, int64_t ws_doubles, float* out, int64_t* counts, void* stream) {
    GEOM_REQUIRE_INPUTS("ncn_geom_loss_fwd");
    NCN_REQUIRE(out != nullptr && counts != nullptr, hipErrorInvalidValue, "ncn_geom_loss_fwd: null output");
    const int nb = geom_blocks(std::max(n_rays, n_tri));
    NCN_REQUIRE(ws != nullptr && ws_doubles >= (int64_t)GM_SUMS * nb, hipErrorInvalidValue,
                "ncn_geom_loss_fwd: workspace of %lld doubles, %lld needed", (long long)ws_doubles,
                (long long)GM_SUMS * nb);
    hipLaunchKernelGGL(geom_fwd_kernel, dim3(nb), dim3(GM_THREADS), 0, (hipStream_t)stream, depth, depth_gt, n_rays,
                       normals, normals_gt, x1, x2, x3, n_tri, terms, step_dev, step, reg_start, ws);
    NCN_LAUNCH_CHECK("ncn_geom_loss_fwd");
    hipLaunchKernelGGL(geom_fwd_reduce_kernel, dim3(1), dim3(GM_THREADS), 0, (hipStream_t)stream, ws, nb, n_tri, terms,
                       w_depth, w_l1, w_dot, step_dev, step, reg_start, out, counts);
    NCN_LAUNCH_CHECK("ncn_geom_loss_fwd (reduce)");
    return 0;
}

int ncn_geom_loss_bwd(const float* depth, const float* depth_gt, int64_t n_rays, const float* normals,
                      const float* normals_gt, const int64_t* x1, const int64_t* x2, const int64_t* x3, int64_t n_tri,
                      const float* rays_o, const float* rays_d, int terms, float w_depth, float w_l1, float w_dot,
                      const int64_t* out_counts, const float* upstream, float* ddepth, float* dn, void* stream) {
    GEOM_REQUIRE_INPUTS("ncn_geom_loss_bwd");
    NCN_REQUIRE((rays_o == nullptr) == (rays_d == nullptr), hipErrorInvalidValue,
                "ncn_geom_loss_bwd: rays_o and rays_d are given together or not at all");
    NCN_REQUIRE(rays_o == nullptr || (dn == nullptr && x2 != nullptr && x3 != nullptr), hipErrorInvalidValue,
                "ncn_geom_loss_bwd: with the rays the normal terms go to ddepth: dn must be NULL, x2 and x3 given");
    NCN_REQUIRE(out_counts != nullptr && upstream != nullptr, hipErrorInvalidValue,
                "ncn_geom_loss_bwd: the forward's counts and the upstream gradients are needed");
    NCN_REQUIRE(dn == nullptr || n_tri == 0 || (normals != nullptr && normals_gt != nullptr && x1 != nullptr),
                hipErrorInvalidValue, "ncn_geom_loss_bwd: dn needs normals, normals_gt and x1");
    const int64_t n = std::max<int64_t>(ddepth != nullptr ? n_rays : 0, dn != nullptr ? n_tri : 0);
    if (n == 0) return 0;
    NCN_REQUIRE(cdiv(std::max(n, n_tri), GM_THREADS) <= 0x7FFFFFFF, hipErrorInvalidValue,
                "ncn_geom_loss_bwd: too many rays");
    // (the kernels read the inputs of a term only where it is in `terms` and live in out_counts)
    hipLaunchKernelGGL(geom_bwd_kernel, dim3((unsigned)cdiv(n, GM_THREADS)), dim3(GM_THREADS), 0, (hipStream_t)stream,
                       depth, depth_gt, n_rays, normals, normals_gt, x1, n_tri, terms, w_depth, w_l1, w_dot, out_counts,
                       upstream, ddepth, dn);
    NCN_LAUNCH_CHECK("ncn_geom_loss_bwd");
    const bool through = rays_o != nullptr && (terms & (NCN_GEOM_NORM_L1 | NCN_GEOM_NORM_DOT));
    if (((terms & NCN_GEOM_REG) || through) && ddepth != nullptr && n_tri > 0) {
        hipLaunchKernelGGL(geom_bwd_scatter_kernel, dim3((unsigned)cdiv(n_tri, GM_THREADS)), dim3(GM_THREADS), 0,
                           (hipStream_t)stream, depth, n_rays, normals, normals_gt, x1, x2, x3, n_tri, rays_o, rays_d,
                           terms, w_l1, w_dot, out_counts, upstream, ddepth);
        NCN_LAUNCH_CHECK("ncn_geom_loss_bwd (scatter)");
    }
    return 0;
}

int ncn_batch_labels_fw(const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_rays, const float* depth,
                        const float* normals, const float* normals_depth, int n_images, int64_t n_pixels,
                        float* out_depth, float* out_normals, float* out_normals_depth, void* stream) {
    NCN_REQUIRE(n_rays >= 0 && n_images >= 1 && n_pixels >= 1, hipErrorInvalidValue, "ncn_batch_labels_fw: bad sizes");
    NCN_REQUIRE((depth == nullptr || out_depth != nullptr) && (normals == nullptr || out_normals != nullptr) &&
                    (normals_depth == nullptr || out_normals_depth != nullptr),
                hipErrorInvalidValue, "ncn_batch_labels_fw: a plane without its output");
    if (n_rays == 0 || (depth == nullptr && normals == nullptr && normals_depth == nullptr)) return 0;
    NCN_REQUIRE(img_idxs != nullptr && pix_idxs != nullptr, hipErrorInvalidValue, "ncn_batch_labels_fw: null indices");
    NCN_REQUIRE(cdiv(n_rays, GM_THREADS) <= 0x7FFFFFFF, hipErrorInvalidValue, "ncn_batch_labels_fw: too many rays");
    hipLaunchKernelGGL(batch_labels_fw_kernel, dim3((unsigned)cdiv(n_rays, GM_THREADS)), dim3(GM_THREADS), 0,
                       (hipStream_t)stream, img_idxs, pix_idxs, n_rays, depth, normals, normals_depth, n_images,
                       n_pixels, out_depth, out_normals, out_normals_depth);
    NCN_LAUNCH_CHECK("ncn_batch_labels_fw");
    return 0;
}

int ncn_batch_semantics_fw(const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_rays, const void* plane,
                           int plane_bytes, int n_images, int64_t n_pixels, int64_t* out, void* stream) {
    NCN_REQUIRE(n_rays >= 0 && n_images >= 1 && n_pixels >= 1, hipErrorInvalidValue, "ncn_batch_semantics_fw: bad sizes");
    NCN_REQUIRE(plane_bytes == 1 || plane_bytes == 4 || plane_bytes == 8, hipErrorInvalidValue,
                "ncn_batch_semantics_fw: plane_bytes = %d; 1 (uint8), 4 (int32) or 8 (int64)", plane_bytes);
    if (n_rays == 0) return 0;
    NCN_REQUIRE(img_idxs != nullptr && pix_idxs != nullptr && plane != nullptr && out != nullptr, hipErrorInvalidValue,
                "ncn_batch_semantics_fw: null argument");
    NCN_REQUIRE(cdiv(n_rays, GM_THREADS) <= 0x7FFFFFFF, hipErrorInvalidValue, "ncn_batch_semantics_fw: too many rays");
    hipLaunchKernelGGL(batch_semantics_fw_kernel, dim3((unsigned)cdiv(n_rays, GM_THREADS)), dim3(GM_THREADS), 0,
                       (hipStream_t)stream, img_idxs, pix_idxs, n_rays, plane, plane_bytes, n_images, n_pixels, out);
    NCN_LAUNCH_CHECK("ncn_batch_semantics_fw");
    return 0;
}

}  // extern "C"
