// Compositing, forward (volumerendering.cu:97-176): row blocks of one wave, the workgroup path of
// long rays, the kernel.
#pragma once
#include "vren_composite.h"

namespace ncn {

// The forward's per-sample arrays of one ray, as buffer descriptors sized to its segment.
struct FwRay {
    __amdgpu_buffer_rsrc_t r_s, r_d, r_t, r_r, r_w;
};
template <int C>
__device__ __forceinline__ FwRay make_fw_ray(const float* __restrict__ sigmas, const float* __restrict__ raws,
                                             const float* __restrict__ deltas, const float* __restrict__ ts,
                                             float* __restrict__ ws, int64_t start, int N) {
    const uint32_t nb = (uint32_t)N * 4u;
    return {buf_rsrc(sigmas + start, nb), buf_rsrc(deltas + start, nb), buf_rsrc(ts + start, nb),
            buf_rsrc(raws + start * C, nb * C), buf_rsrc(ws + start, nb)};
}

// sigma, delta, t and raw of ROWS rows from `base`, every load issued before the first use; past
// the segment the descriptors read 0.
template <int C, int ROWS>
__device__ __forceinline__ void composite_fw_load(const FwRay& y, int base, int lane, float (&sg)[ROWS],
                                                  float (&dl)[ROWS], float (&tt)[ROWS], float (&rr)[ROWS][C]) {
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        const uint32_t k = (uint32_t)(base + r * 64 + lane);
        sg[r] = buf_load(y.r_s, k * 4u);
        dl[r] = buf_load(y.r_d, k * 4u);
        tt[r] = buf_load(y.r_t, k * 4u);
#pragma unroll
        for (int i = 0; i < C; i++) rr[r][i] = buf_load(y.r_r, k * (4u * C) + 4u * i);
    }
}

// One block of a ray's rows (forward).  All of the block's loads are issued up front; the ROWS
// product scans run interleaved in one asm (wave_incl_prod_multi) and only the carries chain
// through readlane.  Returns true when the ray stopped in this block (quirk q6: the stopping sample
// is composited, not counted); the rest of the segment then gets ws = 0 (volumerendering.cu:133
// breaks, ws stays 0).
// LOCAL (the single-wave path of rays longer than 256 samples, guarded 4-row blocks: rows past N are
// skipped): the chain starts at 1 inside the block and is scaled by `carry` (the product of the
// preceding blocks) - the same float operations, in the same order, as the one-workgroup path
// (composite_fw_coop), so a long ray composites bit-identically on either path.
template <int C, int ROWS, bool LOCAL = false>
__device__ __forceinline__ bool composite_fw_block(const FwRay& y, int base, int N, float T_thr, int lane, float& Tc,
                                                   float (&acc)[2 + C], int& total, float carry = 1.0f) {
    float sg[ROWS], dl[ROWS], tt[ROWS], rr[ROWS][C];
    if constexpr (LOCAL) {  // rows past N are skipped (uniform branches)
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const uint32_t k = (uint32_t)(base + r * 64 + lane);
            if (r == 0 || base + r * 64 < N) {
                sg[r] = buf_load(y.r_s, k * 4u);
                dl[r] = buf_load(y.r_d, k * 4u);
                tt[r] = buf_load(y.r_t, k * 4u);
#pragma unroll
                for (int i = 0; i < C; i++) rr[r][i] = buf_load(y.r_r, k * (4u * C) + 4u * i);
            } else {
                sg[r] = dl[r] = 0.f;  // (this order of the three: another one costs composite_fw_kernel<3> 2 SGPRs)
                tt[r] = 0.f;
#pragma unroll
                for (int i = 0; i < C; i++) rr[r][i] = 0.f;
            }
        }
    } else {
        composite_fw_load<C, ROWS>(y, base, lane, sg, dl, tt, rr);
    }
    float a[ROWS], om[ROWS], p[ROWS];
    cf_alpha_scan<ROWS>(sg, dl, a, om, p);
    // transmittance in front of (Tb) and after (Ta) each sample; lanes past N carry the last Ta
    float Tb[ROWS];
    uint64_t stopm[ROWS];
    if constexpr (LOCAL) {
        Tc = cf_local_chain(p, om, Tb);
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            Tb[r] *= carry;
            stopm[r] = __ballot(Tb[r] * om[r] <= T_thr);
        }
    } else {
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            Tb[r] = Tc * wave_shr1_dpp(p[r], 1.0f);
            const float Ta = Tb[r] * om[r];
            stopm[r] = __ballot(Ta <= T_thr);
            Tc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Ta), 63));
        }
    }
    int srow = ROWS, slane = 64;  // first sample whose Ta <= T_thr (T is non-increasing)
#pragma unroll
    for (int r = ROWS - 1; r >= 0; r--)
        if (stopm[r]) {
            srow = r;
            slane = __builtin_ctzll(stopm[r]);
        }
    float w[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        w[r] = (r < srow || (r == srow && lane <= slane)) ? a[r] * Tb[r] : 0.f;
        if (!LOCAL || r == 0 || base + r * 64 < N) buf_store(y.r_w, (uint32_t)(base + r * 64 + lane) * 4u, w[r]);
    }
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        acc[0] += w[r];
        acc[1] = fmaf(w[r], tt[r], acc[1]);
#pragma unroll
        for (int i = 0; i < C; i++) acc[2 + i] = fmaf(w[r], rr[r][i], acc[2 + i]);
    }
    if (srow < ROWS) {
        total = base + srow * 64 + slane;
        for (int k = base + ROWS * 64 + lane; k < N; k += 64) buf_store(y.r_w, (uint32_t)k * 4u, 0.f);
        return true;
    }
    return false;
}

// The per-ray outputs (one lane): acc = {opacity, depth, rend[C]}, total = the samples counted.
template <int C>
__device__ __forceinline__ void composite_fw_store(int64_t ray, const float (&acc)[2 + C], int total,
                                                   int64_t* __restrict__ total_samples, float* __restrict__ opacity,
                                                   float* __restrict__ depth, float* __restrict__ rend, float bg,
                                                   float* __restrict__ rgb_bg) {
    opacity[ray] = acc[0];
    depth[ray] = acc[1];
#pragma unroll
    for (int i = 0; i < C; i++) rend[ray * C + i] = acc[2 + i];
    if (rgb_bg) {  // render()'s background, rendering.py:232-240: rgb = rend + bg * (1 - opacity)
#pragma unroll
        for (int i = 0; i < C; i++) rgb_bg[ray * C + i] = acc[2 + i] + bg * (1 - acc[0]);
    }
    total_samples[ray] = total;
}

// The workgroup path of one long ray (see vren_composite.h).
template <int C>
__device__ __forceinline__ void composite_fw_coop(const float* __restrict__ sigmas, const float* __restrict__ raws,
                                                  const float* __restrict__ deltas, const float* __restrict__ ts,
                                                  const int64_t* __restrict__ rays_a, int64_t row, float T_thr,
                                                  int64_t* __restrict__ total_samples, float* __restrict__ opacity,
                                                  float* __restrict__ depth, float* __restrict__ rend,
                                                  float* __restrict__ ws, float bg, float* __restrict__ rgb_bg) {
    __shared__ float sP[CF_WPB];
    __shared__ int sStop[CF_WPB];
    __shared__ float sAcc[CF_WPB][2 + C];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ray = rays_a[3 * row], start = rays_a[3 * row + 1];
    const int N = (int)rays_a[3 * row + 2];
    if (N <= CF_LONG || N > CF_COOP_MAX) return;  // workgroup-uniform: no wave reaches a barrier
    const FwRay y = make_fw_ray<C>(sigmas, raws, deltas, ts, ws, start, N);
    const int base = wv * 256;
    float sg[4], dl[4], tt[4], rr[4][C];
    composite_fw_load<C, 4>(y, base, lane, sg, dl, tt, rr);  // (whole waves past N read 0 too)
    float a[4], om[4], p[4];
    cf_alpha_scan<4>(sg, dl, a, om, p);
    float Tb[4];
    const float Tc = cf_local_chain(p, om, Tb);
    if (lane == 0) sP[wv] = Tc;
    __syncthreads();
    float carry = 1.0f;
    for (int v = 0; v < wv; v++) carry *= sP[v];
    int stop = INT_MAX;  // first sample (ray position) whose transmittance after it is <= T_thr
#pragma unroll
    for (int r = 3; r >= 0; r--) {
        Tb[r] *= carry;
        const uint64_t m = __ballot(Tb[r] * om[r] <= T_thr);
        if (m) stop = base + r * 64 + __builtin_ctzll(m);
    }
    if (lane == 0) sStop[wv] = stop;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < CF_WPB; v++) stop = min(stop, sStop[v]);
    float acc[2 + C];
#pragma unroll
    for (int i = 0; i < 2 + C; i++) acc[i] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int pos = base + r * 64 + lane;
        const float w = pos <= stop ? a[r] * Tb[r] : 0.f;  // the stopping sample is composited (q6)
        if (base + r * 64 < N) buf_store(y.r_w, (uint32_t)pos * 4u, w);
        acc[0] += w;
        acc[1] = fmaf(w, tt[r], acc[1]);
#pragma unroll
        for (int i = 0; i < C; i++) acc[2 + i] = fmaf(w, rr[r][i], acc[2 + i]);
    }
    wave_sum_multi<2 + C>(acc);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 2 + C; i++) sAcc[wv][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 2 + C; i++) {
            float t = sAcc[0][i];
            for (int v = 1; v < CF_WPB; v++) t += sAcc[v][i];
            acc[i] = t;
        }
        composite_fw_store<C>(ray, acc, stop == INT_MAX ? N : stop, total_samples, opacity, depth, rend, bg, rgb_bg);
    }
}

// Forward (volumerendering.cu:97-176): a ray with N <= 256 samples is one block of 1, 2 or 4 rows
// (every row non-empty: no guards), a longer one runs in guarded 4-row blocks with local chains.
template <int C>
__global__ __launch_bounds__(64 * CF_WPB) void composite_fw_kernel(
    const float* __restrict__ sigmas, const float* __restrict__ raws, const float* __restrict__ deltas,
    const float* __restrict__ ts, const int64_t* __restrict__ rays_a, int64_t R, float T_thr,
    int64_t* __restrict__ total_samples, float* __restrict__ opacity, float* __restrict__ depth,
    float* __restrict__ rend, float* __restrict__ ws, float bg, float* __restrict__ rgb_bg, int n_coop) {
    if ((int)blockIdx.x < n_coop) {
        for (int64_t row = blockIdx.x; cf_long_row(rays_a, R, row); row += n_coop)
            composite_fw_coop<C>(sigmas, raws, deltas, ts, rays_a, row, T_thr, total_samples, opacity, depth, rend,
                                 ws, bg, rgb_bg);
        return;
    }
    const int lane = threadIdx.x & 63;
    bool taken;
    const RaySeg g = cf_own_ray(rays_a, R, n_coop, taken);
    if (taken) return;
    const int N = g.N;
    const FwRay y = make_fw_ray<C>(sigmas, raws, deltas, ts, ws, g.start, N);
    float Tc = 1.0f;
    float acc[2 + C];  // opacity, depth, rend[C]
#pragma unroll
    for (int i = 0; i < 2 + C; i++) acc[i] = 0.f;
    int total = N;
    if (N <= 64) {  // N == 0 included: every load reads 0, every store is dropped
        composite_fw_block<C, 1>(y, 0, N, T_thr, lane, Tc, acc, total);
    } else if (N <= 128) {
        composite_fw_block<C, 2>(y, 0, N, T_thr, lane, Tc, acc, total);
    } else if (N <= 256) {
        composite_fw_block<C, 4>(y, 0, N, T_thr, lane, Tc, acc, total);
    } else {  // 4-row blocks with local chains, block sums added in order (as composite_fw_coop)
        float carry = 1.0f;
        for (int base = 0; base < N; base += 4 * 64) {
            float bacc[2 + C];
#pragma unroll
            for (int i = 0; i < 2 + C; i++) bacc[i] = 0.f;
            const bool stopped = composite_fw_block<C, 4, true>(y, base, N, T_thr, lane, Tc, bacc, total, carry);
            wave_sum_multi<2 + C>(bacc);
#pragma unroll
            for (int i = 0; i < 2 + C; i++) acc[i] += bacc[i];
            carry *= Tc;
            if (stopped) break;
        }
    }
    if (N <= 256) wave_sum_multi<2 + C>(acc);
    if (g.live && lane == 0) composite_fw_store<C>(g.ray, acc, total, total_samples, opacity, depth, rend, bg, rgb_bg);
}

}  // namespace ncn
