// Loss stage 1: normals from rendered depth over pixel triangles (datasets/hypersim_src/utils.py:504-541)
// and their backward to the depth (and, for pose refinement, to the rays).
#pragma once
#include "common.h"

namespace ncn {

// ---- normals: P = o + d*depth ; n = normalize(cross(P2-P1, P3-P1)) (F.normalize eps 1e-12) ----
__device__ __forceinline__ void tri_points(const float* __restrict__ o, const float* __restrict__ d,
                                           const float* __restrict__ depth, int64_t i, float P[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) P[k] = o[3 * i + k] + d[3 * i + k] * depth[i];
}

__device__ __forceinline__ void normals_fwd_one(const float* __restrict__ o, const float* __restrict__ d,
                                                const float* __restrict__ depth, const int64_t* __restrict__ x1,
                                                const int64_t* __restrict__ x2, const int64_t* __restrict__ x3,
                                                int64_t t, float* __restrict__ normals) {
    float P1[3], P2[3], P3[3];
    tri_points(o, d, depth, x1[t], P1);
    tri_points(o, d, depth, x2[t], P2);
    tri_points(o, d, depth, x3[t], P3);
    const float a0 = P2[0] - P1[0], a1 = P2[1] - P1[1], a2 = P2[2] - P1[2];
    const float b0 = P3[0] - P1[0], b1 = P3[1] - P1[1], b2 = P3[2] - P1[2];
    const float c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
    const float nrm = fmaxf(sqrtf(c0 * c0 + c1 * c1 + c2 * c2), 1e-12f);
    normals[3 * t] = c0 / nrm;
    normals[3 * t + 1] = c1 / nrm;
    normals[3 * t + 2] = c2 / nrm;
}

inline __global__ void normals_fwd_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                   const float* __restrict__ depth, const int64_t* __restrict__ x1,
                                   const int64_t* __restrict__ x2, const int64_t* __restrict__ x3, int64_t T,
                                   float* __restrict__ normals) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    normals_fwd_one(o, d, depth, x1, x2, x3, t, normals);
}

// d/d depth through P_k = o + d*depth, a = P2-P1, b = P3-P1, c = a x b, n = c / max(|c|, eps):
// the three vertex gradients (g1, g2, g3) of triangle t for the normal gradient g.
__device__ __forceinline__ void tri_depth_grads(const float* __restrict__ o, const float* __restrict__ d,
                                                const float* __restrict__ depth, int64_t i1, int64_t i2, int64_t i3,
                                                const float g[3], float& g1, float& g2, float& g3) {
    float P1[3], P2[3], P3[3];
    tri_points(o, d, depth, i1, P1);
    tri_points(o, d, depth, i2, P2);
    tri_points(o, d, depth, i3, P3);
    const float a[3] = {P2[0] - P1[0], P2[1] - P1[1], P2[2] - P1[2]};
    const float b[3] = {P3[0] - P1[0], P3[1] - P1[1], P3[2] - P1[2]};
    const float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const float len = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    float dc[3];
    if (len > 1e-12f) {
        const float n[3] = {c[0] / len, c[1] / len, c[2] / len};
        const float ng = n[0] * g[0] + n[1] * g[1] + n[2] * g[2];
#pragma unroll
        for (int k = 0; k < 3; k++) dc[k] = (g[k] - n[k] * ng) / len;
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) dc[k] = g[k] / 1e-12f;
    }
    // c = a x b :  da = b x dc ,  db = dc x a
    const float da[3] = {b[1] * dc[2] - b[2] * dc[1], b[2] * dc[0] - b[0] * dc[2], b[0] * dc[1] - b[1] * dc[0]};
    const float db[3] = {dc[1] * a[2] - dc[2] * a[1], dc[2] * a[0] - dc[0] * a[2], dc[0] * a[1] - dc[1] * a[0]};
    g2 = da[0] * d[3 * i2] + da[1] * d[3 * i2 + 1] + da[2] * d[3 * i2 + 2];
    g3 = db[0] * d[3 * i3] + db[1] * d[3 * i3 + 1] + db[2] * d[3 * i3 + 2];
    g1 = -((da[0] + db[0]) * d[3 * i1] + (da[1] + db[1]) * d[3 * i1 + 1] + (da[2] + db[2]) * d[3 * i1 + 2]);
}
// normal gradient of triangle t: dn (T,3), or with term weights tw the (3,T,3) per-term stack
__device__ __forceinline__ void tri_normal_grad(const float* __restrict__ dn, const float* tw, int64_t T, int64_t t,
                                                float g[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) g[k] = dn[3 * t + k];
    if (tw) {
#pragma unroll
        for (int k = 0; k < 3; k++) g[k] = tw[0] * g[k] + tw[1] * dn[T * 3 + 3 * t + k] + tw[2] * dn[T * 6 + 3 * t + k];
    }
}

inline __global__ void normals_bwd_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                   const float* __restrict__ depth, const int64_t* __restrict__ x1,
                                   const int64_t* __restrict__ x2, const int64_t* __restrict__ x3, int64_t T,
                                   const float* __restrict__ dn, const float* __restrict__ tw,
                                   float* __restrict__ ddepth) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int64_t i1 = x1[t], i2 = x2[t], i3 = x3[t];
    float g[3], g1, g2, g3;
    tri_normal_grad(dn, tw, T, t, g);
    tri_depth_grads(o, d, depth, i1, i2, i3, g, g1, g2, g3);
    atomicAdd(ddepth + i1, g1);
    atomicAdd(ddepth + i2, g2);
    atomicAdd(ddepth + i3, g3);
}

// The same backward with the rays' gradients (camera pose refinement: rays_o / rays_d require
// grad): dL/dP1 = -(da + db), dL/dP2 = da, dL/dP3 = db through P = o + d * depth, so per corner
// dL/do += dL/dP, dL/dd += depth * dL/dP, dL/ddepth += d . dL/dP (the sums of ncn_normals_bwd).
inline __global__ void normals_bwd_rays_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                        const float* __restrict__ depth, const int64_t* __restrict__ x1,
                                        const int64_t* __restrict__ x2, const int64_t* __restrict__ x3, int64_t T,
                                        const float* __restrict__ dn, const float* __restrict__ tw,
                                        float* __restrict__ ddepth, float* __restrict__ d_o, float* __restrict__ d_d) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int64_t idx[3] = {x1[t], x2[t], x3[t]};
    float g[3];
    tri_normal_grad(dn, tw, T, t, g);
    float P1[3], P2[3], P3[3];
    tri_points(o, d, depth, idx[0], P1);
    tri_points(o, d, depth, idx[1], P2);
    tri_points(o, d, depth, idx[2], P3);
    const float a[3] = {P2[0] - P1[0], P2[1] - P1[1], P2[2] - P1[2]};
    const float b[3] = {P3[0] - P1[0], P3[1] - P1[1], P3[2] - P1[2]};
    const float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const float len = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    float dc[3];
    if (len > 1e-12f) {
        const float n[3] = {c[0] / len, c[1] / len, c[2] / len};
        const float ng = n[0] * g[0] + n[1] * g[1] + n[2] * g[2];
#pragma unroll
        for (int k = 0; k < 3; k++) dc[k] = (g[k] - n[k] * ng) / len;
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) dc[k] = g[k] / 1e-12f;
    }
    const float da[3] = {b[1] * dc[2] - b[2] * dc[1], b[2] * dc[0] - b[0] * dc[2], b[0] * dc[1] - b[1] * dc[0]};
    const float db[3] = {dc[1] * a[2] - dc[2] * a[1], dc[2] * a[0] - dc[0] * a[2], dc[0] * a[1] - dc[1] * a[0]};
    const float dP[3][3] = {{-(da[0] + db[0]), -(da[1] + db[1]), -(da[2] + db[2])},
                            {da[0], da[1], da[2]},
                            {db[0], db[1], db[2]}};
#pragma unroll
    for (int v = 0; v < 3; v++) {
        const int64_t i = idx[v];
        const float dep = depth[i];
        atomicAdd(ddepth + i, dP[v][0] * d[3 * i] + dP[v][1] * d[3 * i + 1] + dP[v][2] * d[3 * i + 2]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicAdd(d_o + 3 * i + k, dP[v][k]);
            atomicAdd(d_d + 3 * i + k, dP[v][k] * dep);
        }
    }
}

}  // namespace ncn
