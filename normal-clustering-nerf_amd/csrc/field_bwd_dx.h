#pragma once
#include "field_scatter.h"  // (sc_corner_entries; with field_de_ws.h, field_grid.h)

namespace ncn {
// Encoding input gradient dL/dx (ncn_field_bwd_dx): the derivative of the trilinear interpolation
// contracted with the encoding gradient the MLP pass left in the dE workspace.  Along dimension k
// the interpolation is linear inside a cell, so per level and feature
//   d enc / d x01_k = scale * sum over the 4 corner pairs of the other two dims of
//                     w_other * (T[hi_k] - T[lo_k]),
// piecewise constant along k, with the forward's cell choice (level_pos: the same fmaf / floorf).
// Same shape as the forward: lane (g, r) of a wave takes levels {2g, 2g+1, 8+2g, 9+2g} of the
// sample at processing position r of its group (its dE pairs are the 64 contiguous bytes a row of
// 16 lanes reads per level), two levels' gathers in flight, fp32 accumulation in a fixed order,
// the four row groups summed by two fixed exchanges, one 12-byte store per sample (sample order).
// No atomics: two runs are bit-identical.  Non-finite dE (an overflowed fp16 chain) propagates.
__device__ __forceinline__ float de_value(uint32_t bits16, bool bf16) {
    return bf16 ? __uint_as_float(bits16 << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
}
__device__ __forceinline__ void dx_level(const float2* __restrict__ tab, const LevelTable& L, int l, float x, float y,
                                         float z, uint32_t dE, bool bf16, float (&acc)[3]) {
    const LevelPos p = level_pos(L.scale[l], x, y, z);
    ScLevel sl;
    sl.res = L.res[l]; sl.params = L.params[l];
    sl.dense = (uint64_t)sl.res * sl.res * sl.res <= sl.params;
    uint32_t e[8];
    sc_corner_entries(sl, p.px, p.py, p.pz, e);
    const uint32_t off = L.offset[l];
    float2 v[8];
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] = tab[off + e[c]];
    const float d0 = de_value(dE & 0xFFFFu, bf16), d1 = de_value(dE >> 16, bf16);
    float u[8];  // the corner values contracted with the level's two dE features
#pragma unroll
    for (int c = 0; c < 8; c++) u[c] = fmaf(d1, v[c].y, d0 * v[c].x);
    const float wx[2] = {1.0f - p.fx, p.fx}, wy[2] = {1.0f - p.fy, p.fy}, wz[2] = {1.0f - p.fz, p.fz};
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
        for (int a = 0; a < 2; a++) {
            gx = fmaf(wy[a] * wz[b], u[1 + 2 * a + 4 * b] - u[2 * a + 4 * b], gx);
            gy = fmaf(wx[a] * wz[b], u[a + 2 + 4 * b] - u[a + 4 * b], gy);
            gz = fmaf(wx[a] * wy[b], u[a + 2 * b + 4] - u[a + 2 * b], gz);
        }
    acc[0] = fmaf(L.scale[l], gx, acc[0]);
    acc[1] = fmaf(L.scale[l], gy, acc[1]);
    acc[2] = fmaf(L.scale[l], gz, acc[2]);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void field_bwd_dx_kernel(
    const float* __restrict__ xyzs, int64_t n_cap, const int32_t* __restrict__ n_dev, const int32_t* __restrict__ order,
    const float2* __restrict__ table, LevelTable Lt, float xyz_min, float xyz_extent, const float* __restrict__ dE_ws,
    float* __restrict__ dL_dxyzs) {
    __shared__ LevelTable L;
    load_levels(L, Lt);
    __syncthreads();
    const int64_t n = n_dev ? min<int64_t>(n_cap, *n_dev) : n_cap;
    const DeWs ws(n_cap);  // the MLP pass's workspace (field_de_ws.h): the header and the [16][n_stride] pairs
    const int64_t n_stride = ws.e_stride;
    const float out_scale = dE_ws[DeWs::INV_S] / xyz_extent;  // 1 / S (the chain's scale) and d x01 / d x
    const bool bf16 = dE_ws[DeWs::OPERAND] != 0.f;
    const uint32_t* __restrict__ dE = (const uint32_t*)(dE_ws + ws.row(0));
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    const int64_t n_groups = (n_cap + 15) / 16;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t grp = wave0; grp < n_groups; grp += n_waves) {
        const int64_t pos = grp * 16 + r;
        if (grp * 16 >= n) {  // (uniform) rows past the device count leave as zeros
            if (g < 3 && pos < n_cap) dL_dxyzs[3 * pos + g] = 0.f;
            continue;
        }
        const bool valid = pos < n;
        const int64_t s = valid && order ? (int64_t)order[pos] : pos;
        float x = 0.f, y = 0.f, z = 0.f;
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        if (valid) {
            x = (xyzs[3 * s] - xyz_min) / xyz_extent;
            y = (xyzs[3 * s + 1] - xyz_min) / xyz_extent;
            z = (xyzs[3 * s + 2] - xyz_min) / xyz_extent;
            q[0] = dE[(int64_t)(2 * g) * n_stride + pos];
            q[1] = dE[(int64_t)(2 * g + 1) * n_stride + pos];
            q[2] = dE[(int64_t)(8 + 2 * g) * n_stride + pos];
            q[3] = dE[(int64_t)(9 + 2 * g) * n_stride + pos];
        }
        float acc[3] = {0.f, 0.f, 0.f};
        dx_level(table, L, 2 * g, x, y, z, q[0], bf16, acc);
        dx_level(table, L, 2 * g + 1, x, y, z, q[1], bf16, acc);
        // (as the forward: the last two levels' gathers wait for the first two's results)
        asm volatile("; dx: levels 8+ after 0-7 %1 %2" : "+v"(x) : "v"(acc[0]), "v"(acc[1]));
        dx_level(table, L, 8 + 2 * g, x, y, z, q[2], bf16, acc);
        dx_level(table, L, 9 + 2 * g, x, y, z, q[3], bf16, acc);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            acc[k] += __shfl_xor(acc[k], 16);
            acc[k] += __shfl_xor(acc[k], 32);
        }
        if (pos < n_cap) {  // (a partial last group: its rows past the count are zero too)
            if (g == 0 && valid) {
                dL_dxyzs[3 * s] = acc[0] * out_scale;
                dL_dxyzs[3 * s + 1] = acc[1] * out_scale;
                dL_dxyzs[3 * s + 2] = acc[2] * out_scale;
            } else if (g == 0) {
                dL_dxyzs[3 * pos] = 0.f; dL_dxyzs[3 * pos + 1] = 0.f; dL_dxyzs[3 * pos + 2] = 0.f;
            }
        }
    }
}
}  // namespace ncn
