// Marcher stage 3: from per-ray slab rows to the packed outputs.  Eager: scan + pack; training step:
// place (the second launch of the fused marcher).
#pragma once
#include "vren_march_wave.h"
#include "workgroup.h"

namespace ncn {

// raymarching_train pass 2: exclusive scan of the counts in ray order (one workgroup; replaces the
// atomicAdd start offsets of raymarching.cu:237-241) -> rays_a, counter = {S, R}.
__global__ __launch_bounds__(1024) void march_train_scan_kernel(const int32_t* __restrict__ counts, int64_t R,
                                                                int64_t* __restrict__ rays_a,
                                                                int32_t* __restrict__ counter) {
    __shared__ int wave_tot[16];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int64_t base = 0; base < R; base += 4096) {  // (uniform trip count: the barriers are safe)
        const int64_t i0 = base + (int64_t)tid * 4;
        int c[4];
        int local = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            c[j] = (i0 + j < R) ? counts[i0 + j] : 0;
            local += c[j];
        }
        int run = block_excl_sweep<1024>(local, carry, wave_tot);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t i = i0 + j;
            if (i < R) {
                rays_a[3 * i] = i;
                rays_a[3 * i + 1] = run;
                rays_a[3 * i + 2] = c[j];
            }
            run += c[j];
        }
    }
    if (tid == 0) {
        counter[0] = carry;
        counter[1] = (int32_t)R;
    }
}

// Samples [k0, n) of a ray's slab row to its packed segment at `start`, one wave: coalesced 4-byte
// lanes, the ray direction broadcast into dirs (raymarching.cu:263-268).
__device__ __forceinline__ void copy_slab_row(const float* __restrict__ sx, const float* __restrict__ st,
                                              const float* __restrict__ sd, const float (&d3)[3], int k0, int n,
                                              int64_t start, int lane, float* __restrict__ xyzs,
                                              float* __restrict__ dirs, float* __restrict__ deltas,
                                              float* __restrict__ ts) {
    for (int k = 3 * k0 + lane; k < 3 * n; k += 64) {
        xyzs[3 * start + k] = sx[k];
        dirs[3 * start + k] = d3[k % 3];
    }
    for (int k = k0 + lane; k < n; k += 64) {
        ts[start + k] = st[k];
        deltas[start + k] = sd[k];
    }
}

// raymarching_train pass 3: one wave per ray copies its slab row to the packed outputs
// (coalesced 4-byte lanes) and broadcasts the ray direction into dirs (raymarching.cu:263-268).
__global__ __launch_bounds__(256) void march_train_pack_kernel(
    const float* __restrict__ rays_d, const int64_t* __restrict__ rays_a, int64_t R, int max_samples,
    const float* __restrict__ slab_xyz, const float* __restrict__ slab_t, const float* __restrict__ slab_dt,
    float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas, float* __restrict__ ts) {
    const int lane = threadIdx.x & 63;
    // wave-uniform ray index (readfirstlane: the per-ray loads below become scalar s_loads)
    const int64_t n = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (n >= R) return;
    const int64_t ray = rays_a[3 * n], start = rays_a[3 * n + 1];
    const int cnt = (int)rays_a[3 * n + 2];
    const float d3[3] = {rays_d[3 * ray], rays_d[3 * ray + 1], rays_d[3 * ray + 2]};
    copy_slab_row(slab_xyz + ray * (int64_t)max_samples * 3, slab_t + ray * (int64_t)max_samples,
                  slab_dt + ray * (int64_t)max_samples, d3, 0, cnt, start, lane, xyzs, dirs, deltas, ts);
}

__global__ __launch_bounds__(256) void march_train_place_kernel(
    const float* __restrict__ rays_d, int64_t R, int max_samples, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ wg_sum, const float* __restrict__ slab_xyz, const float* __restrict__ slab_t,
    const float* __restrict__ slab_dt, int64_t* __restrict__ rays_a, float* __restrict__ xyzs,
    float* __restrict__ dirs, float* __restrict__ deltas, float* __restrict__ ts, int32_t* __restrict__ counter) {
    __shared__ int red[4][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x;
    // exclusive prefix over the workgroup sums [0, b) and the total of long rays: 16 loads per
    // thread (every workgroup's word), all in flight
    int v[PLACE_MAX_WG / 256];
#pragma unroll
    for (int u = 0; u < PLACE_MAX_WG / 256; u++) {
        const int i = u * 256 + threadIdx.x;
        v[u] = i < (int)gridDim.x ? wg_sum[i] : 0;
    }
    const int64_t r0 = __builtin_amdgcn_readfirstlane((int)(b * 4 + wv));
    const bool live = r0 < R;
    const int64_t r = live ? r0 : R - 1;
    const int n = live ? counts[r] : 0;
    // the first 256 samples of the ray's slab row are fetched while the prefix is formed
    const float d3[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
    const float* sx = slab_xyz + r * (int64_t)max_samples * 3;
    const float* st = slab_t + r * (int64_t)max_samples;
    const float* sd = slab_dt + r * (int64_t)max_samples;
    constexpr int PF = 4;  // rows of 64 prefetched (xyz: 3 floats per sample -> 3*PF loads)
    float px[3 * PF], pt[PF], pd[PF];
#pragma unroll
    for (int q = 0; q < 3 * PF; q++) px[q] = q * 64 + lane < 3 * n ? sx[q * 64 + lane] : 0.f;
#pragma unroll
    for (int q = 0; q < PF; q++) {
        pt[q] = q * 64 + lane < n ? st[q * 64 + lane] : 0.f;
        pd[q] = q * 64 + lane < n ? sd[q * 64 + lane] : 0.f;
    }
    int pre[3] = {0, 0, 0};  // samples before this workgroup, long rays before it, in all
#pragma unroll
    for (int u = 0; u < PLACE_MAX_WG / 256; u++) {
        const int i = u * 256 + threadIdx.x;
        const int nl = (int)((unsigned)v[u] >> 26);
        if (i < b) {
            pre[0] += v[u] & ((1 << 26) - 1);
            pre[1] += nl;
        }
        pre[2] += nl;
    }
    block_sum<3, 256>(pre, red);
    int start = pre[0];
    const int long_before = pre[1], long_total = pre[2];
    __syncthreads();
    int* const len = &red[0][0];  // (red again, behind the barrier: the four waves' ray lengths)
    if (lane == 0) len[wv] = n;
    __syncthreads();
    int lw = 0;  // long rays among the earlier waves of this workgroup
    for (int w = 0; w < wv; w++) {
        start += len[w];
        lw += len[w] > PLACE_LONG;
    }
    const int64_t row = n > PLACE_LONG ? (int64_t)(long_before + lw)
                                       : (int64_t)long_total + (4 * (int64_t)b - long_before) + (wv - lw);
    if (b == (int)gridDim.x - 1 && threadIdx.x == 0) {
        counter[0] = start + len[0] + len[1] + len[2] + len[3];  // (thread 0: start = the workgroup's prefix)
        counter[1] = (int32_t)R;
    }
    if (!live) return;
    if (lane == 0) {
        rays_a[3 * row] = r;
        rays_a[3 * row + 1] = start;
        rays_a[3 * row + 2] = n;
    }
    float* ox = xyzs + 3 * (int64_t)start;
    float* od = dirs + 3 * (int64_t)start;
#pragma unroll
    for (int q = 0; q < 3 * PF; q++) {
        const int k = q * 64 + lane;
        if (k < 3 * n) {
            ox[k] = px[q];
            od[k] = d3[k % 3];
        }
    }
#pragma unroll
    for (int q = 0; q < PF; q++) {
        const int k = q * 64 + lane;
        if (k < n) {
            ts[start + k] = pt[q];
            deltas[start + k] = pd[q];
        }
    }
    copy_slab_row(sx, st, sd, d3, PF * 64, n, start, lane, xyzs, dirs, deltas, ts);
}

}  // namespace ncn
