// Ray-AABB intersection: the slab test of one box and ray_aabb_intersect over a list of boxes.
#pragma once
#include "common.h"

namespace ncn {

// The slab test of one box (intersection.cu:5-27): entry t1 and exit t2 along the ray (origin o,
// inverse direction inv), both -1 when the ray misses.  The expression order is the oracle's.
__device__ __forceinline__ void slab_test(const float (&o)[3], const float (&inv)[3], const float* __restrict__ c,
                                          const float* __restrict__ hs, float& t1, float& t2) {
    float a1[3], a2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float tmin = (c[k] - hs[k] - o[k]) * inv[k];
        const float tmax = (c[k] + hs[k] - o[k]) * inv[k];
        a1[k] = fminf(tmin, tmax);
        a2[k] = fmaxf(tmin, tmax);
    }
    t1 = fmaxf(fmaxf(a1[0], a1[1]), a1[2]);
    t2 = fminf(fminf(a2[0], a2[1]), a2[2]);
    if (t1 > t2) { t1 = -1.0f; t2 = -1.0f; }
}

// ray_aabb_intersect (intersection.cu:5-56 + :95-97 sort): one lane per ray, voxels in order,
// slots sorted stably by t1 (empty slots carry t1 = -1 and therefore sort first, as torch::sort does).
template <int MAXH>
__global__ __launch_bounds__(256) void ray_aabb_kernel(const float* __restrict__ rays_o,
                                                       const float* __restrict__ rays_d, int64_t R,
                                                       const float* __restrict__ centers,
                                                       const float* __restrict__ half_sizes, int64_t V, int max_hits,
                                                       int32_t* __restrict__ hit_cnt, float* __restrict__ hits_t,
                                                       int64_t* __restrict__ hits_idx, float near_distance) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float o[3] = {rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2]};
    float inv[3] = {1.0f / rays_d[3 * r], 1.0f / rays_d[3 * r + 1], 1.0f / rays_d[3 * r + 2]};
    float h1[MAXH], h2[MAXH];
    int64_t hv[MAXH];
#pragma unroll
    for (int k = 0; k < MAXH; k++) { h1[k] = -1.0f; h2[k] = -1.0f; hv[k] = -1; }
    int cnt = 0;
    for (int64_t v = 0; v < V; v++) {
        float t1, t2;
        slab_test(o, inv, centers + 3 * v, half_sizes + 3 * v, t1, t2);
        if (t2 > 0) {
            if (cnt < max_hits) {
#pragma unroll
                for (int k = 0; k < MAXH; k++)
                    if (k == cnt) { h1[k] = fmaxf(t1, 0.0f); h2[k] = t2; hv[k] = v; }
            }
            cnt++;
        }
    }
    // stable insertion sort of the max_hits slots by t1
    for (int i = 1; i < max_hits; i++) {
        for (int j = i; j > 0; j--) {
            if (h1[j - 1] > h1[j]) {
                float a = h1[j]; h1[j] = h1[j - 1]; h1[j - 1] = a;
                float b = h2[j]; h2[j] = h2[j - 1]; h2[j - 1] = b;
                int64_t c = hv[j]; hv[j] = hv[j - 1]; hv[j - 1] = c;
            } else {
                break;
            }
        }
    }
    hit_cnt[r] = cnt;
    // render()'s near clamp of the first hit (rendering.py:28), fused: t1 in [0, near) -> near
    if (h1[0] >= 0.0f && h1[0] < near_distance) h1[0] = near_distance;
    for (int k = 0; k < max_hits; k++) {
        hits_t[(r * max_hits + k) * 2] = h1[k];
        hits_t[(r * max_hits + k) * 2 + 1] = h2[k];
        hits_idx[r * max_hits + k] = hv[k];
    }
}

}  // namespace ncn
