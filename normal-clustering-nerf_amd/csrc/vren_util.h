// Occupancy utilities and per-step reductions: morton kernels, packbits, the sample count, the
// marcher backward's segment sums.
#pragma once
#include "vren_march.h"
#include "workgroup.h"

namespace ncn {

// raymarching.cu:62-70, 90-101, 122-141
__global__ void morton3D_kernel(const int32_t* __restrict__ c, int64_t n, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = (int32_t)morton3D((uint32_t)c[3 * i], (uint32_t)c[3 * i + 1], (uint32_t)c[3 * i + 2]);
}
__global__ void morton3D_invert_kernel(const int32_t* __restrict__ idx, int64_t n, int32_t* __restrict__ c) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t ind = idx[i];
    c[3 * i + 0] = (int32_t)morton3D_invert((uint32_t)(ind >> 0));
    c[3 * i + 1] = (int32_t)morton3D_invert((uint32_t)(ind >> 1));
    c[3 * i + 2] = (int32_t)morton3D_invert((uint32_t)(ind >> 2));
}
// total_samples.sum() of VolumeRenderer.forward (custom_functions.py:139-146) in one workgroup,
// optionally adding the marcher's count and that sum into a running f64 pair (throughput counters
// that stay on the device: no per-step copies).
__global__ __launch_bounds__(1024) void count_samples_kernel(const int64_t* __restrict__ total, int64_t R,
                                                             const int32_t* __restrict__ counter,
                                                             int64_t* __restrict__ sum_out, double* __restrict__ acc) {
    count_samples_wg(total, R, counter, sum_out, acc);
}

__global__ void packbits_kernel(const float4* __restrict__ grid, int64_t n_bytes, float thr,
                                uint8_t* __restrict__ bitfield) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_bytes) return;
    const float4 lo = grid[2 * n], hi = grid[2 * n + 1];
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) bits |= (v[i] > thr) ? (1u << i) : 0u;
    bitfield[n] = (uint8_t)bits;
}

// RayMarcher.backward (custom_functions.py:102-112): torch_scatter.segment_csr over
// indptr = [rays_a[:, 1], rays_a[-1, 1] + rays_a[-1, 2]], so row r sums samples
// [rays_a[r, 1], rays_a[r + 1, 1]) (the last row up to its start + count; an inverted range sums to 0):
//   dL/drays_o[r] = sum dL/dxyzs,   dL/drays_d[r] = sum (dL/dxyzs * ts + dL/ddirs).
// One wave per row, no atomics: lane l adds samples l, l + 64, ... in order, then the fixed
// permlane/DPP tree of wave_sum_multi — the summation order depends only on the segment, so
// repeated launches are bit-identical.  The d-term is rounded as the reference's torch ops round it
// (a product, then a sum: no fma contraction).  gx / gd may be NULL (that gradient is zero).
__global__ __launch_bounds__(256) void segment_csr_kernel(const float* __restrict__ gx, const float* __restrict__ gd,
                                                          const float* __restrict__ ts,
                                                          const int64_t* __restrict__ rays_a, int64_t R,
                                                          float* __restrict__ d_o, float* __restrict__ d_d) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int64_t start = rays_a[3 * r + 1];
    const int64_t end = (r + 1 < R) ? rays_a[3 * (r + 1) + 1] : start + rays_a[3 * r + 2];
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t s = start + lane; s < end; s += 64) {
        const float t = ts[s];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float x = gx ? gx[3 * s + c] : 0.f;
            const float y = gd ? gd[3 * s + c] : 0.f;
            a[c] = a[c] + x;
            a[3 + c] = a[3 + c] + ((x * t) + y);
        }
    }
    wave_sum_multi<6>(a);
    if (lane < 3) {
        const float vo = lane == 0 ? a[0] : (lane == 1 ? a[1] : a[2]);
        const float vd = lane == 0 ? a[3] : (lane == 1 ? a[4] : a[5]);
        d_o[3 * r + lane] = vo;
        d_d[3 * r + lane] = vd;
    }
}

}  // namespace ncn
