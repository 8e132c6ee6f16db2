// Loss stage 2: photometric MSE + opacity entropy, forward (alone, or beside the normals and the
// sample count in one launch) and backward, and the fused backward of the reference configuration.
#pragma once
#include "loss_normals.h"
#include "workgroup.h"

namespace ncn {

// ---- photometric MSE + opacity entropy (losses.py:349-362, validity filter :246-262) ----
// One workgroup: loss[0] = mean((rgb - gt)^2), loss[1] = w_op * mean(-o log o), o = opacity + 1e-10.
constexpr int PH_THREADS = 1024;
__device__ __forceinline__ void photo_loss_fwd_wg(const float* __restrict__ rgb, const float* __restrict__ gt,
                                                  const float* __restrict__ op, int64_t R, float w_op,
                                                  float* __restrict__ loss) {
    __shared__ float red[PH_THREADS / 64][2];
    float s[2] = {0.f, 0.f};  // (accumulators that start at +0 are never -0: the sums need no 0 in front)
    for (int64_t i = threadIdx.x; i < R; i += PH_THREADS) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float d = rgb[3 * i + c] - gt[3 * i + c];
            s[0] += d * d;
        }
        const float o = op[i] + 1e-10f;
        s[1] += -o * logf(o);
    }
    block_sum<2, PH_THREADS>(s, red);
    if (threadIdx.x == 0) {
        const float mse = s[0] / (float)(3 * R), ent = w_op * (s[1] / (float)R);
        loss[0] = isfinite(mse) ? mse : 0.f;  // validity filter
        loss[1] = isfinite(ent) ? ent : 0.f;
        loss[2] = isfinite(mse) ? 1.f : 0.f;
        loss[3] = isfinite(ent) ? 1.f : 0.f;
    }
}

inline __global__ __launch_bounds__(PH_THREADS) void photo_loss_fwd_kernel(const float* __restrict__ rgb,
                                                                    const float* __restrict__ gt,
                                                                    const float* __restrict__ op, int64_t R,
                                                                    float w_op, float* __restrict__ loss) {
    photo_loss_fwd_wg(rgb, gt, op, R, w_op, loss);
}

// The photometric/opacity reduction (workgroup 0) and the normals from depth (the other
// workgroups, one triangle per thread) in one launch: the two independent forward parts of the
// fused loss node.
// With cnt_total: one more workgroup (block 1) sums the compositor's per-ray sample counts (the
// vr_samples of the render, ncn_count_samples' work) beside them instead of in a launch of its own.
// (workgroup bid of the launch; a device function so that a wider launch can append workgroups of
// its own behind these, split_fused.hip)
__device__ __forceinline__ void photo_normals_fwd_wg(
    const int bid, const float* __restrict__ rgb, const float* __restrict__ gt, const float* __restrict__ op, int64_t R,
    float w_op, float* __restrict__ loss, const float* __restrict__ o, const float* __restrict__ d,
    const float* __restrict__ depth, const int64_t* __restrict__ x1, const int64_t* __restrict__ x2,
    const int64_t* __restrict__ x3, int64_t T, float* __restrict__ normals, const int64_t* __restrict__ cnt_total,
    int64_t cnt_n, const int32_t* __restrict__ cnt_counter, int64_t* __restrict__ cnt_out, double* __restrict__ cnt_acc) {
    if (bid == 0) {
        photo_loss_fwd_wg(rgb, gt, op, R, w_op, loss);
        return;
    }
    const int nb0 = cnt_total ? 2 : 1;  // workgroups in front of the normals
    if (cnt_total && bid == 1) {
        count_samples_wg(cnt_total, cnt_n, cnt_counter, cnt_out, cnt_acc);
        return;
    }
    const int64_t t = (int64_t)(bid - nb0) * PH_THREADS + threadIdx.x;
    if (t < T) normals_fwd_one(o, d, depth, x1, x2, x3, t, normals);
}
inline __global__ __launch_bounds__(PH_THREADS) void photo_normals_fwd_kernel(
    const float* __restrict__ rgb, const float* __restrict__ gt, const float* __restrict__ op, int64_t R, float w_op,
    float* __restrict__ loss, const float* __restrict__ o, const float* __restrict__ d,
    const float* __restrict__ depth, const int64_t* __restrict__ x1, const int64_t* __restrict__ x2,
    const int64_t* __restrict__ x3, int64_t T, float* __restrict__ normals, const int64_t* __restrict__ cnt_total,
    int64_t cnt_n, const int32_t* __restrict__ cnt_counter, int64_t* __restrict__ cnt_out, double* __restrict__ cnt_acc) {
    photo_normals_fwd_wg((int)blockIdx.x, rgb, gt, op, R, w_op, loss, o, d, depth, x1, x2, x3, T, normals, cnt_total,
                         cnt_n, cnt_counter, cnt_out, cnt_acc);
}
// dL/drgb of one channel: ga = the upstream gradient times the term's validity flag, sa = 2 / (3 R)
__device__ __forceinline__ float photo_drgb(float ga, float sa, float rgb, float gt) {
    return ga == 0.f ? 0.f : ga * sa * (rgb - gt);
}
// grads scaled by the upstream gradient g[0..1] (device scalars) and zeroed for filtered terms
inline __global__ void photo_loss_bwd_kernel(const float* __restrict__ rgb, const float* __restrict__ gt,
                                      const float* __restrict__ op, int64_t R, float w_op,
                                      const float* __restrict__ loss, const float* __restrict__ g,
                                      float* __restrict__ drgb, float* __restrict__ dop) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const float ga = g ? g[0] * loss[2] : loss[2], gb = g ? g[1] * loss[3] : loss[3];
    const float sa = 2.f / (float)(3 * R);
#pragma unroll
    for (int c = 0; c < 3; c++) drgb[3 * i + c] = ga == 0.f ? 0.f : ga * sa * (rgb[3 * i + c] - gt[3 * i + c]);
    const float o = op[i] + 1e-10f;
    dop[i] = gb == 0.f ? 0.f : gb * w_op * (-(logf(o) + 1.f)) / (float)R;  // filtered term: no NaN leaks
}

// ---- fused backward of NeRFMTLoss for the reference configuration (losses.py:349-362 + 420-478,
// `all_images_triang_patch` 8x8 patches, base.py:53-58 / losses.py:307-313): one thread per ray
// writes dL/drgb and dL/dopacity of the photometric terms and GATHERS dL/ddepth from the (at most
// three) patch triangles the ray is a vertex of, so no zero-fill and no atomics:
//   local (i,j) is x1 of triangle (i,j) [i,j >= 1], x2 of (i+1,j) [i <= 6, j >= 1], x3 of (i,j+1)
//   [i >= 1, j <= 6]; triangle (i,j) of patch p is index p*49 + 7(i-1) + (j-1).
// Upstream gradients: up_total (the `total` output) + up_terms[5] (rgb, opacity, ort, centr_dot,
// centr_L1 outputs), either may be NULL (= 0).
inline __global__ void nerf_loss_bwd_kernel(const float* __restrict__ rgb, const float* __restrict__ gt,
                                     const float* __restrict__ op, int64_t R, float w_op,
                                     const float* __restrict__ photo, const float* __restrict__ o,
                                     const float* __restrict__ d, const float* __restrict__ depth,
                                     const float* __restrict__ dn, const float* __restrict__ up_total,
                                     const float* __restrict__ up_terms, float* __restrict__ drgb,
                                     float* __restrict__ dop, float* __restrict__ ddepth) {
    const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ray >= R) return;
    const float ut = up_total ? *up_total : 0.f;
    float u[5];
#pragma unroll
    for (int q = 0; q < 5; q++) u[q] = ut + (up_terms ? up_terms[q] : 0.f);
    // photometric (photo_loss_bwd_kernel)
    if (drgb) {
        const float ga = u[0] * photo[2], gb = u[1] * photo[3];
        const float sa = 2.f / (float)(3 * R);
#pragma unroll
        for (int c = 0; c < 3; c++) drgb[3 * ray + c] = photo_drgb(ga, sa, rgb[3 * ray + c], gt[3 * ray + c]);
        const float oo = op[ray] + 1e-10f;
        dop[ray] = gb == 0.f ? 0.f : gb * w_op * (-(logf(oo) + 1.f)) / (float)R;
    }
    if (!ddepth) return;
    // normals -> depth, gathered over this ray's triangle roles
    const int64_t T = (R / 64) * 49;
    const float tw[3] = {u[2], u[3], u[4]};
    const int64_t p = ray >> 6;
    const int loc = (int)(ray & 63), i = loc >> 3, j = loc & 7;
    const int64_t b = p * 64;
    float acc = 0.f;
    float g[3], g1, g2, g3;
    if (i >= 1 && j >= 1) {  // x1 of (i, j)
        const int64_t t = p * 49 + 7 * (i - 1) + (j - 1);
        tri_normal_grad(dn, tw, T, t, g);
        tri_depth_grads(o, d, depth, ray, b + 8 * (i - 1) + j, b + 8 * i + (j - 1), g, g1, g2, g3);
        acc += g1;
    }
    if (i <= 6 && j >= 1) {  // x2 of (i+1, j)
        const int64_t t = p * 49 + 7 * i + (j - 1);
        tri_normal_grad(dn, tw, T, t, g);
        tri_depth_grads(o, d, depth, b + 8 * (i + 1) + j, ray, b + 8 * (i + 1) + (j - 1), g, g1, g2, g3);
        acc += g2;
    }
    if (i >= 1 && j <= 6) {  // x3 of (i, j+1)
        const int64_t t = p * 49 + 7 * (i - 1) + j;
        tri_normal_grad(dn, tw, T, t, g);
        tri_depth_grads(o, d, depth, b + 8 * i + (j + 1), b + 8 * (i - 1) + (j + 1), ray, g, g1, g2, g3);
        acc += g3;
    }
    ddepth[ray] = acc;
}

}  // namespace ncn
