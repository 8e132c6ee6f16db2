// Device-resident training data: the patch sampler, the ray generator and the backward into the
// per-image pose corrections dR (axis-angle) / dT.
//  * ncn_batch_draw     <- datasets/base.py:142-167 (the two *_triang_patch strategies)
//  * ncn_batch_rays_fw  <- datasets/base.py:176-177 + train_nerf.py:167-182 (poses[img_idxs],
//                          directions[pix_idxs], axisangle_to_R (ray_utils.py:75-101), get_rays
//                          (ray_utils.py:45-71))
//  * ncn_batch_rays_bw  <- autograd of train_nerf.py:177-182 into self.dR / self.dT (:244-249)
// All three read no host value but their arguments, allocate nothing and never synchronise, so they
// can be nodes of a captured step.  An index outside its range (img_idxs / pix_idxs filled by a
// caller) gives NaN outputs, never an out-of-bounds access.
#include "workgroup.h"
#include "../../include/ncnerf.h"

#include <math.h>

namespace ncn {

// ---- sampler ---------------------------------------------------------------------------------
// splitmix64 output of the counter k under `seed`: the state seed + k * golden gamma through the
// finaliser (the mixer of the marcher's jitter, vren_march_wave.h: march_uniform, restated here).
__device__ __forceinline__ uint64_t splitmix64_at(uint64_t seed, uint64_t k) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * k;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the counter of (step, r): distinct for distinct pairs with r < 2^32 (0x100000001B3 > 2^32)
__device__ __forceinline__ uint64_t counter_key(uint64_t step, uint64_t r) { return step * 0x100000001B3ull + r; }

// Integer draw in [0, n): the high 64 bits of z * n (bias n * 2^-64).
__device__ __forceinline__ uint64_t draw_below(uint64_t z, uint64_t n) { return __umul64hi(z, n); }

__global__ __launch_bounds__(256) void batch_draw_kernel(uint64_t seed, const int64_t* __restrict__ step_dev,
                                                         int64_t step_host, int n_images, int H, int W, int patch,
                                                         int64_t n_patches, int same_image, int corner_mode,
                                                         int64_t* __restrict__ img_idxs,
                                                         int64_t* __restrict__ pix_idxs) {
    const int area = patch * patch;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_patches * area) return;
    const uint64_t step = (uint64_t)(step_dev ? *step_dev : step_host);
    const uint64_t p = (uint64_t)(i / area);
    const int cell = (int)(i % area), iy = cell / patch, ix = cell % patch;
    // counters: 0 = the one image of a same-image batch, 1 + 2 p + s = stream s of patch p
    const uint64_t zi = splitmix64_at(seed, counter_key(step, same_image ? 0 : 1 + 2 * p));
    const uint64_t zc = splitmix64_at(seed, counter_key(step, 2 + 2 * p));
    const int cw = W - patch + 1;
    const int64_t c = (int64_t)draw_below(zc, (uint64_t)(H - patch + 1) * (uint64_t)cw);
    img_idxs[i] = (int64_t)draw_below(zi, (uint64_t)n_images);
    // corner_mode 0: the offsets are added to the corner's ORDINAL (base.py:164-166); 1: to the corner
    pix_idxs[i] = corner_mode == 0 ? c + (int64_t)iy * W + ix : (c / cw + iy) * W + c % cw + ix;
}

// ---- pose correction -------------------------------------------------------------------------
// axisangle_to_R (ray_utils.py:75-101): A = I + a K + b K^2, K = skew(v), theta = |v| + 1e-7,
// a = sin(theta) / theta, b = (1 - cos(theta)) / theta^2.  b is evaluated as sinc(theta / 2)^2 / 2,
// which has no cancellation (the plain fp32 form is 0 below theta = 2.4e-4); a needs no care
// (theta >= 1e-7).
struct AxisAngle {
    float th, a, b;
};
__device__ __forceinline__ AxisAngle axis_angle_coeffs(const float v[3]) {
    AxisAngle c;
    c.th = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-7f;
    c.a = sinf(c.th) / c.th;
    const float h = 0.5f * c.th, s = sinf(h) / h;
    c.b = 0.5f * s * s;
    return c;
}
// K = skew(v) row-major
__device__ __forceinline__ void skew(const float v[3], float K[9]) {
    K[0] = 0.f, K[1] = -v[2], K[2] = v[1];
    K[3] = v[2], K[4] = 0.f, K[5] = -v[0];
    K[6] = -v[1], K[7] = v[0], K[8] = 0.f;
}
__device__ __forceinline__ void mat3_mul(const float A[9], const float B[9], float C[9]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void axis_angle_matrix(const float v[3], float A[9]) {
    const AxisAngle c = axis_angle_coeffs(v);
    float K[9], K2[9];
    skew(v, K);
    mat3_mul(K, K, K2);
#pragma unroll
    for (int k = 0; k < 9; k++) A[k] = ((k & 3) == 0 ? 1.f : 0.f) + c.a * K[k] + c.b * K2[k];
}

template <typename T>
__device__ __forceinline__ float pixel_value(T v);
template <>
__device__ __forceinline__ float pixel_value<float>(float v) { return v; }
template <>
__device__ __forceinline__ float pixel_value<uint8_t>(uint8_t v) { return (float)v / 255.0f; }

// One thread per ray.  The rotation of a ray's image (A(dR[i]) R_i, 27 multiply-adds) is formed per
// ray: cheaper than a launch that forms it per image first.
template <typename T>
__global__ __launch_bounds__(256) void batch_rays_fw_kernel(
    const int64_t* __restrict__ img_idxs, const int64_t* __restrict__ pix_idxs, int64_t R, const T* __restrict__ images,
    const float* __restrict__ directions, const float* __restrict__ poses, const float* __restrict__ dR,
    const float* __restrict__ dT, int n_images, int64_t HW, float* __restrict__ rays_o, float* __restrict__ rays_d,
    float* __restrict__ rgb) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int64_t im = img_idxs[r], px = pix_idxs[r];
    if (im < 0 || im >= n_images || px < 0 || px >= HW) {
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < 3; k++) {
            rays_o[3 * r + k] = nan;
            rays_d[3 * r + k] = nan;
            rgb[3 * r + k] = nan;
        }
        return;
    }
    const float* P = poses + im * 12;  // (3,4) row-major: [R | t]
    float Rm[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        Rm[3 * i] = P[4 * i], Rm[3 * i + 1] = P[4 * i + 1], Rm[3 * i + 2] = P[4 * i + 2];
        t[i] = P[4 * i + 3];
    }
    if (dR) {  // R' = A(dR[i]) R_i, t' = t_i + dT[i]  (train_nerf.py:178-180)
        const float v[3] = {dR[3 * im], dR[3 * im + 1], dR[3 * im + 2]};
        float A[9], R2[9];
        axis_angle_matrix(v, A);
        mat3_mul(A, Rm, R2);
#pragma unroll
        for (int k = 0; k < 9; k++) Rm[k] = R2[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] += dT[3 * im + k];
    }
    const float d[3] = {directions[3 * px], directions[3 * px + 1], directions[3 * px + 2]};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        rays_d[3 * r + i] = Rm[3 * i] * d[0] + Rm[3 * i + 1] * d[1] + Rm[3 * i + 2] * d[2];
        rays_o[3 * r + i] = t[i];
    }
    const T* src = images + (im * HW + px) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) rgb[3 * r + k] = pixel_value<T>(src[k]);
}

// d theta-coefficients / d theta: a' = (theta cos - sin) / theta^2, b' = (theta sin - 2 (1 - cos)) /
// theta^3.  Both cancel at small theta (the numerators are O(theta^3), O(theta^4) differences of
// O(theta), O(theta^2) terms): below 0.5 their series, truncated at a relative theta^8 / 1.3e6 < 3e-9.
__device__ __forceinline__ void axis_angle_dcoeffs(float th, float& da, float& db) {
    if (th < 0.5f) {
        const float t2 = th * th;
        da = th * (-1.f / 3.f + t2 * (1.f / 30.f + t2 * (-1.f / 840.f + t2 * (1.f / 45360.f))));
        db = th * (-1.f / 12.f + t2 * (1.f / 180.f + t2 * (-1.f / 6720.f + t2 * (1.f / 453600.f))));
    } else {
        const float s = sinf(th), c = cosf(th);
        da = (th * c - s) / (th * th);
        db = (th * s - 2.f * (1.f - c)) / (th * th * th);
    }
}

constexpr int BW_THREADS = 256;
// One workgroup per image: its threads scan all R rays in a fixed assignment (ray r -> thread r %
// 256, ascending), so the 12 sums — G = sum g_d (x) (R_i dir) and sum g_o — have one summation order
// whatever the order of img_idxs: no float atomics, two runs are bit-identical.  Thread 0 then
// contracts G with dA/dv_k.  Every row of grad_dR / grad_dT is written (zeros for absent images).
__global__ __launch_bounds__(BW_THREADS) void batch_rays_bw_kernel(
    const float* __restrict__ g_o, const float* __restrict__ g_d, const int64_t* __restrict__ img_idxs,
    const int64_t* __restrict__ pix_idxs, int64_t R, const float* __restrict__ directions,
    const float* __restrict__ poses, const float* __restrict__ dR, int64_t HW, float* __restrict__ grad_dR,
    float* __restrict__ grad_dT) {
    __shared__ float part[BW_THREADS / 64][12];
    const int64_t im = blockIdx.x;
    const float* P = poses + im * 12;
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.f;
    for (int64_t r = threadIdx.x; r < R; r += BW_THREADS) {
        if (img_idxs[r] != im) continue;
        const int64_t px = pix_idxs[r];
        float u[3];
        if (px < 0 || px >= HW) {
            u[0] = u[1] = u[2] = __builtin_nanf("");
        } else {
            const float d[3] = {directions[3 * px], directions[3 * px + 1], directions[3 * px + 2]};
#pragma unroll
            for (int i = 0; i < 3; i++) u[i] = P[4 * i] * d[0] + P[4 * i + 1] * d[1] + P[4 * i + 2] * d[2];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float gd = g_d[3 * r + i];
#pragma unroll
            for (int j = 0; j < 3; j++) acc[3 * i + j] += gd * u[j];
            acc[9 + i] += g_o[3 * r + i];
        }
    }
    // (block_sum<12>'s order, written out: through block_sum the outputs came out with other bits
    // (profiles/workgroup/ab_outputs.txt) although the sums' order is the same — thread 0's tail below
    // then compiles differently; how its a * b + c * d sums are contracted is the suspect, unproven)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const float s = wave_sum(acc[k]);
        if (lane == 0) part[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float G[12];
#pragma unroll
    for (int k = 0; k < 12; k++) {
        float s = part[0][k];
        for (int w = 1; w < BW_THREADS / 64; w++) s += part[w][k];
        G[k] = s;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) grad_dT[3 * im + k] = G[9 + k];
    // dL/dv_k = <G, dA/dv_k>,  dA/dv_k = a' t_k K + a E_k + b' t_k K^2 + b (E_k K + K E_k),
    // E_k = skew(e_k), t_k = d theta / d v_k = v_k / |v| (0 at v = 0: torch's norm backward)
    const float v[3] = {dR[3 * im], dR[3 * im + 1], dR[3 * im + 2]};
    const AxisAngle c = axis_angle_coeffs(v);
    float da, db;
    axis_angle_dcoeffs(c.th, da, db);
    const float nv = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    float K[9], K2[9];
    skew(v, K);
    mat3_mul(K, K, K2);
    float gK = 0.f, gK2 = 0.f;  // <G, K>, <G, K^2>
#pragma unroll
    for (int k = 0; k < 9; k++) {
        gK += G[k] * K[k];
        gK2 += G[k] * K2[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float e[3] = {k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f};
        float E[9], EK[9], KE[9];
        skew(e, E);
        mat3_mul(E, K, EK);
        mat3_mul(K, E, KE);
        float gE = 0.f, gS = 0.f;
#pragma unroll
        for (int q = 0; q < 9; q++) {
            gE += G[q] * E[q];
            gS += G[q] * (EK[q] + KE[q]);
        }
        const float tk = nv > 0.f ? v[k] / nv : 0.f;
        grad_dR[3 * im + k] = tk * (da * gK + db * gK2) + c.a * gE + c.b * gS;
    }
}

}  // namespace ncn

using namespace ncn;

extern "C" {

int ncn_batch_draw(uint64_t seed, const int64_t* step_dev, int64_t step, int n_images, int H, int W, int patch,
                   int64_t n_patches, int same_image, int corner_mode, int64_t* img_idxs, int64_t* pix_idxs,
                   void* stream) {
    NCN_REQUIRE(n_images >= 1 && H >= 1 && W >= 1, hipErrorInvalidValue, "ncn_batch_draw: bad shape: %d images of %dx%d",
                n_images, H, W);
    NCN_REQUIRE(patch >= 1 && patch <= H && patch <= W && patch <= 1024, hipErrorInvalidValue,
                "ncn_batch_draw: patch %d does not fit a %dx%d image", patch, H, W);
    NCN_REQUIRE((int64_t)H * W < (1ll << 40), hipErrorInvalidValue, "ncn_batch_draw: image too large");
    NCN_REQUIRE(corner_mode == NCN_CORNER_REFERENCE || corner_mode == NCN_CORNER_GRID, hipErrorInvalidValue,
                "ncn_batch_draw: corner_mode %d", corner_mode);
    NCN_REQUIRE(n_patches >= 0 && n_patches < (1ll << 31), hipErrorInvalidValue, "ncn_batch_draw: n_patches %lld",
                (long long)n_patches);
    const int64_t n = n_patches * patch * patch;
    if (n == 0) return 0;
    NCN_REQUIRE(img_idxs && pix_idxs, hipErrorInvalidValue, "ncn_batch_draw: null output");
    NCN_REQUIRE(cdiv(n, 256) <= 0x7FFFFFFF, hipErrorInvalidValue, "ncn_batch_draw: too many rays");
    hipLaunchKernelGGL(batch_draw_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, seed,
                       step_dev, step, n_images, H, W, patch, n_patches, same_image != 0, corner_mode, img_idxs,
                       pix_idxs);
    NCN_LAUNCH_CHECK("ncn_batch_draw");
    return 0;
}

int ncn_batch_rays_fw(const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_rays, const void* images,
                      int image_dtype, const float* directions, const float* poses, const float* dR, const float* dT,
                      int n_images, int64_t n_pixels, float* rays_o, float* rays_d, float* rgb, void* stream) {
    NCN_REQUIRE(n_rays >= 0 && n_images >= 1 && n_pixels >= 1, hipErrorInvalidValue, "ncn_batch_rays_fw: bad sizes");
    NCN_REQUIRE((dR == nullptr) == (dT == nullptr), hipErrorInvalidValue,
                "ncn_batch_rays_fw: dR and dT are given together or not at all");
    NCN_REQUIRE(image_dtype == NCN_IMAGE_F32 || image_dtype == NCN_IMAGE_U8, hipErrorInvalidValue,
                "ncn_batch_rays_fw: image_dtype %d", image_dtype);
    if (n_rays == 0) return 0;
    NCN_REQUIRE(img_idxs && pix_idxs && images && directions && poses && rays_o && rays_d && rgb,
                hipErrorInvalidValue, "ncn_batch_rays_fw: null buffer");
    NCN_REQUIRE(cdiv(n_rays, 256) <= 0x7FFFFFFF, hipErrorInvalidValue, "ncn_batch_rays_fw: too many rays");
    const dim3 grid((unsigned)cdiv(n_rays, 256));
    if (image_dtype == NCN_IMAGE_U8)
        hipLaunchKernelGGL(batch_rays_fw_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, img_idxs, pix_idxs,
                           n_rays, (const uint8_t*)images, directions, poses, dR, dT, n_images, n_pixels, rays_o, rays_d,
                           rgb);
    else
        hipLaunchKernelGGL(batch_rays_fw_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, img_idxs, pix_idxs,
                           n_rays, (const float*)images, directions, poses, dR, dT, n_images, n_pixels, rays_o, rays_d,
                           rgb);
    NCN_LAUNCH_CHECK("ncn_batch_rays_fw");
    return 0;
}

int ncn_batch_rays_bw(const float* dL_drays_o, const float* dL_drays_d, const int64_t* img_idxs,
                      const int64_t* pix_idxs, int64_t n_rays, const float* directions, const float* poses,
                      const float* dR, int n_images, int64_t n_pixels, float* grad_dR, float* grad_dT, void* stream) {
    NCN_REQUIRE(n_rays >= 0 && n_images >= 1 && n_pixels >= 1, hipErrorInvalidValue, "ncn_batch_rays_bw: bad sizes");
    NCN_REQUIRE(directions && poses && dR && grad_dR && grad_dT, hipErrorInvalidValue, "ncn_batch_rays_bw: null buffer");
    NCN_REQUIRE(n_rays == 0 || (dL_drays_o && dL_drays_d && img_idxs && pix_idxs), hipErrorInvalidValue,
                "ncn_batch_rays_bw: null buffer");
    hipLaunchKernelGGL(batch_rays_bw_kernel, dim3((unsigned)n_images), dim3(BW_THREADS), 0, (hipStream_t)stream,
                       dL_drays_o, dL_drays_d, img_idxs, pix_idxs, n_rays, directions, poses, dR, n_pixels, grad_dR,
                       grad_dT);
    NCN_LAUNCH_CHECK("ncn_batch_rays_bw");
    return 0;
}

}  // extern "C"
