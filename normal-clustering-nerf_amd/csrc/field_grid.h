// The multiresolution hash grid: level table, tiny-cuda-nn's index, trilinear encoding of one level.
#pragma once
#include "common.h"
namespace ncn {
struct LevelTable {
    float scale[16];
    uint32_t res[16], params[16], offset[16];
};

// tiny-cuda-nn grid_index (dense stride while it fits, else coherent prime hash) % params
__device__ __forceinline__ uint32_t grid_index(uint32_t params, uint32_t res, uint32_t x, uint32_t y, uint32_t z) {
    uint32_t stride = 1, index = 0;
    if (stride <= params) { index += x * stride; stride *= res; }
    if (stride <= params) { index += y * stride; stride *= res; }
    if (stride <= params) { index += z * stride; stride *= res; }
    if (params < stride) index = x ^ (y * 2654435761u) ^ (z * 805459861u);
    // index % params without a 32-bit division: a hashed level always has params = 2^log2_T (a
    // power of two), a dense level has index < res^3 <= params.  Same result as the modulo.
    if ((params & (params - 1)) == 0) return index & (params - 1);
    return index < params ? index : index % params;
}

struct LevelPos {
    uint32_t px, py, pz;
    float fx, fy, fz;
};
__device__ __forceinline__ LevelPos level_pos(float scale, float x, float y, float z) {
    LevelPos p;
    float a = fmaf(scale, x, 0.5f), b = fmaf(scale, y, 0.5f), c = fmaf(scale, z, 0.5f);
    const float fa = floorf(a), fb = floorf(b), fc = floorf(c);
    p.px = (uint32_t)(int)fa; p.py = (uint32_t)(int)fb; p.pz = (uint32_t)(int)fc;
    p.fx = a - fa; p.fy = b - fb; p.fz = c - fc;
    return p;
}

// trilinear interpolation of one level (tcnn kernel_grid: corner bit d -> +1 along dim d).  Entry
// indices without per-corner grid_index branches: a dense level (res^3 <= params: tcnn's stride
// never exceeds params) is base + dx + dy*res + dz*res^2 (mod params only at the boundary corner
// res^3 == params can't reach: kept as in grid_index), a hashed one ((x+dx) ^ (y+dy)*P1 ^
// (z+dz)*P2) & (params-1) with the four products formed once (params is 2^19 on every hashed
// level).  Corner weights in the association ((wx * wy) * wz) of the reference loop.
__device__ __forceinline__ float2 encode_level(const float2* __restrict__ tab, const LevelTable& L, int l, float x,
                                               float y, float z) {
    const LevelPos p = level_pos(L.scale[l], x, y, z);
    const uint32_t params = L.params[l], res = L.res[l], off = L.offset[l];
    uint32_t e[8];
    if ((uint64_t)res * res * res <= params) {
        const uint32_t b0 = p.px + res * p.py + res * res * p.pz;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const uint32_t i = b0 + (c & 1) + ((c >> 1) & 1) * res + ((c >> 2) & 1) * res * res;
            e[c] = i < params ? i : i % params;
        }
    } else {
        const uint32_t hy0 = p.py * 2654435761u, hy1 = (p.py + 1) * 2654435761u;
        const uint32_t hz0 = p.pz * 805459861u, hz1 = (p.pz + 1) * 805459861u;
        const uint32_t mask = params - 1;
#pragma unroll
        for (int c = 0; c < 8; c++) e[c] = ((p.px + (c & 1)) ^ ((c & 2) ? hy1 : hy0) ^ ((c & 4) ? hz1 : hz0)) & mask;
    }
    float2 v[8];
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] = tab[off + e[c]];
    const float wx[2] = {1.0f - p.fx, p.fx}, wy[2] = {1.0f - p.fy, p.fy}, wz[2] = {1.0f - p.fz, p.fz};
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const float w = (wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2];
        acc.x = fmaf(w, v[c].x, acc.x);
        acc.y = fmaf(w, v[c].y, acc.y);
    }
    return acc;
}

__device__ __forceinline__ void load_levels(LevelTable& Ls, const LevelTable& La) {
    if (threadIdx.x < 16) {
        const int l = threadIdx.x;
        Ls.scale[l] = La.scale[l];
        Ls.res[l] = La.res[l];
        Ls.params[l] = La.params[l];
        Ls.offset[l] = La.offset[l];
    }
}
}  // namespace ncn
