// Marcher stage 1: morton codes, mip levels, the marcher constants, one occupancy probe, the
// empty-voxel skip, and the serial walks (one lane per ray) of raymarching_train and raymarching_test.
#pragma once
#include "common.h"

#define SQRT3 1.73205080757f

namespace ncn {

__device__ __forceinline__ float clampf_(float f, float a, float b) { return fmaxf(a, fminf(f, b)); }
__device__ __forceinline__ float signf_(float x) { return copysignf(1.0f, x); }

__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
// raymarching.cu:44-50
__device__ __forceinline__ uint32_t morton3D(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2);
}
// raymarching.cu:52-60
__device__ __forceinline__ uint32_t morton3D_invert(uint32_t x) {
    x = x & 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}

// raymarching.cu:19-32
__device__ __forceinline__ int mip_from_pos(float x, float y, float z, int cascades) {
    const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    int e;
    frexpf(mx, &e);
    return min(cascades - 1, max(0, e + 1));
}
__device__ __forceinline__ int mip_from_dt(float dt, int grid_size, int cascades) {
    int e;
    frexpf(dt * (float)grid_size, &e);
    return min(cascades - 1, max(0, e));
}

// Marcher constants.  calc_dt (raymarching.cu:11-13) = clamp(t*esf, SQRT3/max_samples, SQRT3*2*scale/G)
struct MarchConst {
    float esf, dt_min, dt_max, scale, gsi;
    int cascades, G, max_samples;
    uint32_t G3;
};
__device__ __forceinline__ MarchConst make_march_const(int cascades, float scale, float esf, int G, int max_samples,
                                                       float dt_scale) {
    MarchConst m;
    m.esf = esf;
    m.dt_min = SQRT3 / (float)max_samples;
    m.dt_max = SQRT3 * 2 * dt_scale / (float)G;
    m.scale = scale;
    m.gsi = 1.0f / (float)G;
    m.cascades = cascades;
    m.G = G;
    m.max_samples = max_samples;
    m.G3 = (uint32_t)G * G * G;
    return m;
}
__device__ __forceinline__ float calc_dt(const MarchConst& m, float t) { return clampf_(t * m.esf, m.dt_min, m.dt_max); }

// One occupancy probe at t (raymarching.cu:205-220).  Returns the voxel (nx,ny,nz), mip bound and
// the bitfield index; `cache_bi/cache_b` memoise the last bitfield byte (same byte => same bits).
template <bool ONE_CASCADE>
__device__ __forceinline__ bool probe(const MarchConst& m, const uint8_t* __restrict__ bitfield, float x, float y,
                                      float z, float dt, int& nx, int& ny, int& nz, float& mip_bound,
                                      uint32_t& cache_bi, uint32_t& cache_b) {
    int mip;
    if (ONE_CASCADE) {
        mip = 0;  // min(cascades-1, ...) == 0 for both mip_from_pos and mip_from_dt
    } else {
        mip = max(mip_from_pos(x, y, z, m.cascades), mip_from_dt(dt, m.G, m.cascades));
    }
    mip_bound = fminf(scalbnf(1.0f, mip - 1), m.scale);
    const float mip_bound_inv = 1.0f / mip_bound;
    nx = (int)clampf_(0.5f * fmaf(x, mip_bound_inv, 1.0f) * (float)m.G, 0.0f, m.G - 1.0f);
    ny = (int)clampf_(0.5f * fmaf(y, mip_bound_inv, 1.0f) * (float)m.G, 0.0f, m.G - 1.0f);
    nz = (int)clampf_(0.5f * fmaf(z, mip_bound_inv, 1.0f) * (float)m.G, 0.0f, m.G - 1.0f);
    const uint32_t idx = (uint32_t)mip * m.G3 + morton3D((uint32_t)nx, (uint32_t)ny, (uint32_t)nz);
    const uint32_t bi = idx >> 3;
    if (bi != cache_bi) {
        cache_b = bitfield[bi];
        cache_bi = bi;
    }
    return (cache_b >> (idx & 7)) & 1u;
}

// Where the skip of an empty probe at t aims (raymarching.cu:224-229): the far face of its voxel.
__device__ __forceinline__ float skip_target(const MarchConst& m, float t, float x, float y, float z, float dx,
                                             float dy, float dz, float dxi, float dyi, float dzi, int nx, int ny,
                                             int nz, float mip_bound) {
    const float tx = fmaf(fmaf(0.5f, signf_(dx), (float)nx + 0.5f) * m.gsi * 2 - 1, mip_bound, -x) * dxi;
    const float ty = fmaf(fmaf(0.5f, signf_(dy), (float)ny + 0.5f) * m.gsi * 2 - 1, mip_bound, -y) * dyi;
    const float tz = fmaf(fmaf(0.5f, signf_(dz), (float)nz + 0.5f) * m.gsi * 2 - 1, mip_bound, -z) * dzi;
    return t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
}

// Empty-voxel skip (raymarching.cu:224-233).
__device__ __forceinline__ float skip_voxel(const MarchConst& m, float t, float x, float y, float z, float dx,
                                            float dy, float dz, float dxi, float dyi, float dzi, int nx, int ny,
                                            int nz, float mip_bound) {
    const float t_target = skip_target(m, t, x, y, z, dx, dy, dz, dxi, dyi, dzi, nx, ny, nz, mip_bound);
    do {
        t += calc_dt(m, t);
    } while (t < t_target);
    return t;
}

// ---------------------------------------------------------------------------------------------
// raymarching_train pass 1: one lane per ray walks it once (raymarching.cu:184-234) and writes the
// samples into its slab row.  64-lane workgroups spread the (latency-bound) walks over the CUs.
template <bool ONE_CASCADE>
__global__ __launch_bounds__(64) void march_train_walk_kernel(
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ hits_t,
    const float* __restrict__ noise, int64_t R, const uint8_t* __restrict__ bitfield, int cascades, float scale,
    float esf, int G, int max_samples, int32_t* __restrict__ counts, float* __restrict__ slab_xyz,
    float* __restrict__ slab_t, float* __restrict__ slab_dt) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const MarchConst m = make_march_const(cascades, scale, esf, G, max_samples, scale);
    const float ox = rays_o[3 * r], oy = rays_o[3 * r + 1], oz = rays_o[3 * r + 2];
    const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float dxi = 1.0f / dx, dyi = 1.0f / dy, dzi = 1.0f / dz;
    float t1 = hits_t[2 * r];
    const float t2 = hits_t[2 * r + 1];
    if (t1 >= 0) {  // :195-198
        const float dt = calc_dt(m, t1);
        t1 = fmaf(dt, noise[r], t1);
    }
    float* sx = slab_xyz + r * (int64_t)max_samples * 3;
    float* st = slab_t + r * (int64_t)max_samples;
    float* sd = slab_dt + r * (int64_t)max_samples;
    uint32_t cache_bi = 0xFFFFFFFFu, cache_b = 0;
    float t = t1;
    int n = 0;
    while (0 <= t && t < t2 && n < max_samples) {  // :204
        const float x = fmaf(t, dx, ox), y = fmaf(t, dy, oy), z = fmaf(t, dz, oz);
        const float dt = calc_dt(m, t);
        int nx, ny, nz;
        float mip_bound;
        if (probe<ONE_CASCADE>(m, bitfield, x, y, z, dt, nx, ny, nz, mip_bound, cache_bi, cache_b)) {
            sx[3 * n] = x;
            sx[3 * n + 1] = y;
            sx[3 * n + 2] = z;
            st[n] = t;
            sd[n] = dt;
            t += dt;
            n++;
        } else {
            t = skip_voxel(m, t, x, y, z, dx, dy, dz, dxi, dyi, dzi, nx, ny, nz, mip_bound);
        }
    }
    counts[r] = n;
}

// raymarching_test (raymarching.cu:335-404): one lane per alive ray; writes all N_samples slots
// (zeros past n_eff, as the torch::zeros outputs of :422-427).  Quirk q3: calc_dt receives
// `cascades` as its scale (:370, :399).
template <bool ONE_CASCADE>
__global__ __launch_bounds__(64) void march_test_kernel(const float* __restrict__ rays_o,
                                                        const float* __restrict__ rays_d, float* __restrict__ hits_t,
                                                        const int64_t* __restrict__ alive, int64_t A,
                                                        const uint8_t* __restrict__ bitfield, int cascades,
                                                        float scale, float esf, int G, int max_samples, int NS,
                                                        float* __restrict__ xyzs, float* __restrict__ dirs,
                                                        float* __restrict__ deltas, float* __restrict__ ts,
                                                        int32_t* __restrict__ n_eff, const int32_t* __restrict__ ctrl) {
    if (ctrl) {  // (device-driven test loop) alive count and samples per ray of this iteration
        A = ctrl[0];
        NS = ctrl[1];
    }
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= A) return;
    const MarchConst m = make_march_const(cascades, scale, esf, G, max_samples, (float)cascades);
    const int64_t r = alive[n];
    const float ox = rays_o[3 * r], oy = rays_o[3 * r + 1], oz = rays_o[3 * r + 2];
    const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float dxi = 1.0f / dx, dyi = 1.0f / dy, dzi = 1.0f / dz;
    float t = hits_t[2 * r];
    const float t2 = hits_t[2 * r + 1];
    float* X = xyzs + n * (int64_t)NS * 3;
    float* D = dirs + n * (int64_t)NS * 3;
    float* DT = deltas + n * (int64_t)NS;
    float* TS = ts + n * (int64_t)NS;
    uint32_t cache_bi = 0xFFFFFFFFu, cache_b = 0;
    int s = 0;
    while (t < t2 && s < NS) {
        const float x = fmaf(t, dx, ox), y = fmaf(t, dy, oy), z = fmaf(t, dz, oz);
        const float dt = calc_dt(m, t);
        int nx, ny, nz;
        float mip_bound;
        if (probe<ONE_CASCADE>(m, bitfield, x, y, z, dt, nx, ny, nz, mip_bound, cache_bi, cache_b)) {
            X[3 * s] = x; X[3 * s + 1] = y; X[3 * s + 2] = z;
            D[3 * s] = dx; D[3 * s + 1] = dy; D[3 * s + 2] = dz;
            TS[s] = t;
            DT[s] = dt;
            t += dt;
            hits_t[2 * r] = t;
            s++;
        } else {
            t = skip_voxel(m, t, x, y, z, dx, dy, dz, dxi, dyi, dzi, nx, ny, nz, mip_bound);
        }
    }
    for (int k = s; k < NS; k++) {
        X[3 * k] = 0.f; X[3 * k + 1] = 0.f; X[3 * k + 2] = 0.f;
        D[3 * k] = 0.f; D[3 * k + 1] = 0.f; D[3 * k + 2] = 0.f;
        TS[k] = 0.f;
        DT[k] = 0.f;
    }
    n_eff[n] = s;
}

}  // namespace ncn
