// Compositing, backward (volumerendering.cu:297-418): row blocks of one wave, the workgroup path of
// long rays, the kernel.
#pragma once
#include "vren_composite.h"

namespace ncn {

// Backward, one block of a ray's rows (volumerendering.cu:297-364).  T is the post-update
// transmittance (quirk q10); d/r are inclusive prefix sums of w*t and w*raw; (sum - pre[s]) is the
// suffix of dL_dws*ws over the WHOLE marched segment (:331-335).  Evaluation order of dL_dsigmas
// follows :349-359.  All of the block's loads are issued up front; the product scans run
// interleaved, the prefix sums of (w*t, w*raw_0..2) as one 4-way DPP scan per row; carries chain
// through readlane.  DWS: a non-NULL dL_dws (the reference's is a zero tensor in training, q5).
// DSIG = false (the split step's early dL/draws, split_fused.hip): only dL_draws = dL_drend * w is
// formed — the dL/dsigma terms, their loads (ts, raws) and their stores are compiled out; w itself
// (alpha, the transmittance chain, the stop) is the same code.
template <int C, int ROWS, bool GUARD, bool DWS, bool DSIG = true>
__device__ __forceinline__ bool composite_bw_block(
    const __amdgpu_buffer_rsrc_t& r_s, const __amdgpu_buffer_rsrc_t& r_d, const __amdgpu_buffer_rsrc_t& r_t,
    const __amdgpu_buffer_rsrc_t& r_r, const __amdgpu_buffer_rsrc_t& r_dw, const __amdgpu_buffer_rsrc_t& r_ws,
    const __amdgpu_buffer_rsrc_t& r_gs, const __amdgpu_buffer_rsrc_t& r_gr, int base, int N, float T_thr,
    int lane, float gO, float dD, float D, float tot, const float (&dR)[C], const float (&RE)[C], float& Tc,
    float& cd, float& cpw, float (&cr)[C]) {
    float sg[ROWS], dl[ROWS], tt[ROWS], rr[ROWS][C], dws[ROWS], pw[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        const uint32_t k = (uint32_t)(base + r * 64 + lane);
        if (!GUARD || r == 0 || base + r * 64 < N) {
            sg[r] = buf_load(r_s, k * 4u);
            dl[r] = buf_load(r_d, k * 4u);
            tt[r] = DSIG ? buf_load(r_t, k * 4u) : 0.f;
#pragma unroll
            for (int i = 0; i < C; i++) rr[r][i] = DSIG ? buf_load(r_r, k * (4u * C) + 4u * i) : 0.f;
            dws[r] = DWS ? buf_load(r_dw, k * 4u) : 0.f;
            pw[r] = DWS ? dws[r] * buf_load(r_ws, k * 4u) : 0.f;
        } else {
            sg[r] = dl[r] = tt[r] = dws[r] = pw[r] = 0.f;
#pragma unroll
            for (int i = 0; i < C; i++) rr[r][i] = 0.f;
        }
    }
    float a[ROWS], om[ROWS], p[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        a[r] = 1.0f - __expf(-sg[r] * dl[r]);
        om[r] = p[r] = 1.0f - a[r];
    }
    wave_incl_prod_multi<ROWS>(p);
    float Tb[ROWS], Ta[ROWS];
    uint64_t stopm[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        Tb[r] = Tc * wave_shr1_dpp(p[r], 1.0f);
        Ta[r] = Tb[r] * om[r];
        stopm[r] = __ballot(Ta[r] <= T_thr);
        Tc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Ta[r]), 63));
    }
    int srow = ROWS, slane = 64;
#pragma unroll
    for (int r = ROWS - 1; r >= 0; r--)
        if (stopm[r]) {
            srow = r;
            slane = __builtin_ctzll(stopm[r]);
        }
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        const bool inc = r < srow || (r == srow && lane <= slane);
        const float w = inc ? a[r] * Tb[r] : 0.f;
        if constexpr (!DSIG) {
            if (!GUARD || r == 0 || base + r * 64 < N) {
#pragma unroll
                for (int i = 0; i < C; i++) buf_store(r_gr, (uint32_t)(base + r * 64 + lane) * (4u * C) + 4u * i, dR[i] * w);
            }
            continue;
        }
        // inclusive prefixes (this row + carry) of w*t, w*raw_i, dL_dws*ws
        // (this row body is composite_bw_coop's too: as one forceinline function it moved four register lines, <1, false> 58 -> 64 VGPRs)
        float run_d = w * tt[r], run_r[C];
#pragma unroll
        for (int i = 0; i < C; i++) run_r[i] = w * rr[r][i];
        if constexpr (C == 3) {
            wave_incl_sum4(run_d, run_r[0], run_r[1], run_r[2]);
        } else {
            run_d = wave_incl_sum_dpp(run_d);
#pragma unroll
            for (int i = 0; i < C; i++) run_r[i] = wave_incl_sum_dpp(run_r[i]);
        }
        run_d += cd;
#pragma unroll
        for (int i = 0; i < C; i++) run_r[i] += cr[i];
        const float run_pw = DWS ? cpw + wave_incl_sum_dpp(pw[r]) : 0.f;
        float gs = gO + dD * (tt[r] * Ta[r] - (D - run_d)) + Ta[r] * dws[r] - (tot - run_pw);
        const bool live_row = !GUARD || r == 0 || base + r * 64 < N;
#pragma unroll
        for (int i = 0; i < C; i++) {
            gs += dR[i] * (rr[r][i] * Ta[r] - (RE[i] - run_r[i]));
            if (live_row) buf_store(r_gr, (uint32_t)(base + r * 64 + lane) * (4u * C) + 4u * i, dR[i] * w);
        }
        if (live_row) buf_store(r_gs, (uint32_t)(base + r * 64 + lane) * 4u, inc ? gs * dl[r] : 0.f);
        cd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run_d), 63));
        if (DWS) cpw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run_pw), 63));
#pragma unroll
        for (int i = 0; i < C; i++) cr[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run_r[i]), 63));
    }
    if (srow < ROWS) {  // rest of the segment: zero gradients
        for (int k = base + ROWS * 64 + lane; k < N; k += 64) {
            if (DSIG) buf_store(r_gs, (uint32_t)k * 4u, 0.f);
#pragma unroll
            for (int i = 0; i < C; i++) buf_store(r_gr, (uint32_t)k * (4u * C) + 4u * i, 0.f);
        }
        return true;
    }
    return false;
}

// Backward (volumerendering.cu:297-418): same block structure as the forward (1/2/4-row blocks for
// N <= 256, guarded 4-row blocks beyond).  A NULL upstream gradient skips its term.
// (DSIG = false: dL_drend is the ray's C values themselves, not the per-ray array, and only sigmas,
// deltas and dL_draws are touched)
template <int C, bool DWS, bool DSIG = true>
__device__ __forceinline__ void composite_bw_ray(
    const float* __restrict__ dL_dopacity, const float* __restrict__ dL_ddepth, const float* __restrict__ dL_drend,
    const float* __restrict__ dL_dws, const float* __restrict__ sigmas, const float* __restrict__ raws,
    const float* __restrict__ ws, const float* __restrict__ deltas, const float* __restrict__ ts, const RaySeg& g,
    const float* __restrict__ opacity, const float* __restrict__ depth, const float* __restrict__ rend,
    float T_thr, float* __restrict__ dL_dsigmas, float* __restrict__ dL_draws, float bg) {
    static_assert(DSIG || !DWS, "the draws-only form has no dL_dws term");
    const int lane = threadIdx.x & 63;
    const int N = g.N;
    const int64_t ray = g.ray;
    // (this per-ray prologue is composite_bw_coop's too: behind one struct + loader <3, false> went from 99 to 95 SGPRs)
    const float dO = DSIG && dL_dopacity ? dL_dopacity[ray] : 0.f;
    const float dD = DSIG && dL_ddepth ? dL_ddepth[ray] : 0.f;
    const float O = DSIG ? opacity[ray] : 0.f, D = DSIG ? depth[ray] : 0.f;
    float dR[C], RE[C];
#pragma unroll
    for (int i = 0; i < C; i++) {
        dR[i] = !DSIG ? dL_drend[i] : dL_drend ? dL_drend[ray * C + i] : 0.f;
        RE[i] = DSIG ? rend[ray * C + i] : 0.f;
    }
    // with the background folded in (rgb = rend + bg * (1 - O)): dL/drend = dL/drgb and the opacity
    // picks up -bg * sum_i dL/drgb_i (the reference's autograd through rendering.py:236)
    float dOe = dO;
    if (bg != 0.f) {
#pragma unroll
        for (int i = 0; i < C; i++) dOe -= bg * dR[i];
    }
    const float gO = dOe * (1 - O);
    const uint32_t nb = (uint32_t)N * 4u;
    const auto r_s = buf_rsrc(sigmas + g.start, nb), r_d = buf_rsrc(deltas + g.start, nb);
    const auto r_gr = buf_rsrc(dL_draws + g.start * C, nb * C);
    const auto r_t = DSIG ? buf_rsrc(ts + g.start, nb) : r_s, r_r = DSIG ? buf_rsrc(raws + g.start * C, nb * C) : r_s;
    const auto r_gs = DSIG ? buf_rsrc(dL_dsigmas + g.start, nb) : r_gr;  // (DSIG = false: never used)
    const auto r_dw = buf_rsrc(DWS ? dL_dws + g.start : dL_dsigmas, DWS ? nb : 0u);
    const auto r_ws = buf_rsrc(DWS ? ws + g.start : dL_dsigmas, DWS ? nb : 0u);
    float tot = 0.f;  // sum of dL_dws * ws over the whole segment
    if (DWS) {
        for (int k = lane; k < N; k += 64) tot = fmaf(buf_load(r_dw, k * 4u), buf_load(r_ws, k * 4u), tot);
        tot = wave_sum_dpp(tot);
    }
    float Tc = 1.0f, cd = 0.f, cpw = 0.f, cr[C];
#pragma unroll
    for (int i = 0; i < C; i++) cr[i] = 0.f;
#define NCN_BW_BLOCK(ROWS, GUARD, BASE)                                                                    \
    composite_bw_block<C, ROWS, GUARD, DWS, DSIG>(r_s, r_d, r_t, r_r, r_dw, r_ws, r_gs, r_gr, BASE, N, T_thr, lane, \
                                                  gO, dD, D, tot, dR, RE, Tc, cd, cpw, cr)
    if (N <= 64) {
        NCN_BW_BLOCK(1, false, 0);
    } else if (N <= 128) {
        NCN_BW_BLOCK(2, false, 0);
    } else if (N <= 256) {
        NCN_BW_BLOCK(4, false, 0);
    } else {
        for (int base = 0; base < N; base += 4 * 64)
            if (NCN_BW_BLOCK(4, true, base)) break;
    }
#undef NCN_BW_BLOCK
}

// Long rays in the backward: one workgroup per ray as in the forward.  Phase 1: every wave loads
// its 256 samples and publishes its local transmittance product and its local sums of w*t, w*raw
// (w with a carry-in of 1) and dL_dws*ws; after one barrier wave v has the carries of the waves in
// front of it (T_in = product of their products; prefix sums = their sums scaled by their T_in;
// the stop cannot lie in front of the first stopping wave, so their sums are uncut), finds its
// first stop, and after a second barrier the ray's first stop cuts w as in the single-wave rows.
// (DSIG = false: as composite_bw_ray's; the first CF_WPB waves of the workgroup take the ray)
template <int C, bool DWS, bool DSIG = true>
__device__ __forceinline__ void composite_bw_coop(
    const float* __restrict__ dL_dopacity, const float* __restrict__ dL_ddepth, const float* __restrict__ dL_drend,
    const float* __restrict__ dL_dws, const float* __restrict__ sigmas, const float* __restrict__ raws,
    const float* __restrict__ ws, const float* __restrict__ deltas, const float* __restrict__ ts,
    const int64_t* __restrict__ rays_a, int64_t row, const float* __restrict__ opacity,
    const float* __restrict__ depth, const float* __restrict__ rend, float T_thr, float* __restrict__ dL_dsigmas,
    float* __restrict__ dL_draws, float bg) {
    __shared__ float sS[CF_WPB][3 + C];  // product, sum w*t, sum dL_dws*ws, sums w*raw
    __shared__ int sStop[CF_WPB];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ray = rays_a[3 * row], start = rays_a[3 * row + 1];
    const int N = (int)rays_a[3 * row + 2];
    if (N <= CF_LONG || N > CF_COOP_MAX) return;  // workgroup-uniform
    // (the per-ray prologue of composite_bw_ray: see there)
    const float dO = DSIG && dL_dopacity ? dL_dopacity[ray] : 0.f;
    const float dD = DSIG && dL_ddepth ? dL_ddepth[ray] : 0.f;
    const float O = DSIG ? opacity[ray] : 0.f, D = DSIG ? depth[ray] : 0.f;
    float dR[C], RE[C];
#pragma unroll
    for (int i = 0; i < C; i++) {
        dR[i] = !DSIG ? dL_drend[i] : dL_drend ? dL_drend[ray * C + i] : 0.f;
        RE[i] = DSIG ? rend[ray * C + i] : 0.f;
    }
    float dOe = dO;
    if (bg != 0.f) {
#pragma unroll
        for (int i = 0; i < C; i++) dOe -= bg * dR[i];
    }
    const float gO = dOe * (1 - O);
    const uint32_t nb = (uint32_t)N * 4u;
    const auto r_s = buf_rsrc(sigmas + start, nb), r_d = buf_rsrc(deltas + start, nb);
    const auto r_gr = buf_rsrc(dL_draws + start * C, nb * C);
    const auto r_t = DSIG ? buf_rsrc(ts + start, nb) : r_s, r_r = DSIG ? buf_rsrc(raws + start * C, nb * C) : r_s;
    const auto r_gs = DSIG ? buf_rsrc(dL_dsigmas + start, nb) : r_gr;  // (DSIG = false: never used)
    const auto r_dw = buf_rsrc(DWS ? dL_dws + start : dL_dsigmas, DWS ? nb : 0u);
    const auto r_ws = buf_rsrc(DWS ? ws + start : dL_dsigmas, DWS ? nb : 0u);
    const int base = wv * 256;
    float sg[4], dl[4], tt[4], rr[4][C], dws[4], pw[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t k = (uint32_t)(base + r * 64 + lane);
        sg[r] = buf_load(r_s, k * 4u);
        dl[r] = buf_load(r_d, k * 4u);
        tt[r] = DSIG ? buf_load(r_t, k * 4u) : 0.f;
#pragma unroll
        for (int i = 0; i < C; i++) rr[r][i] = DSIG ? buf_load(r_r, k * (4u * C) + 4u * i) : 0.f;
        dws[r] = DWS ? buf_load(r_dw, k * 4u) : 0.f;
        pw[r] = DWS ? dws[r] * buf_load(r_ws, k * 4u) : 0.f;
    }
    float a[4], om[4], p[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        a[r] = 1.0f - __expf(-sg[r] * dl[r]);
        om[r] = p[r] = 1.0f - a[r];
    }
    wave_incl_prod_multi<4>(p);
    float Tb[4], Tl = 1.0f, ls[2 + C];  // local sums: w*t, dL_dws*ws, w*raw
#pragma unroll
    for (int i = 0; i < 2 + C; i++) ls[i] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        Tb[r] = Tl * wave_shr1_dpp(p[r], 1.0f);
        Tl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Tb[r] * om[r]), 63));
        if constexpr (!DSIG) continue;  // (only the product is carried)
        const float w = a[r] * Tb[r];
        ls[0] = fmaf(w, tt[r], ls[0]);
        ls[1] += pw[r];
#pragma unroll
        for (int i = 0; i < C; i++) ls[2 + i] = fmaf(w, rr[r][i], ls[2 + i]);
    }
    if constexpr (DSIG) wave_sum_multi<2 + C>(ls);
    if (lane == 0) {
        sS[wv][0] = Tl;
#pragma unroll
        for (int i = 0; i < 2 + C; i++) sS[wv][1 + i] = ls[i];
    }
    __syncthreads();
    float Tc = 1.0f, cd = 0.f, cpw = 0.f, tot = 0.f, cr[C];
#pragma unroll
    for (int i = 0; i < C; i++) cr[i] = 0.f;
    for (int v = 0; v < CF_WPB; v++) {
        if (v < wv) {
            cd = fmaf(Tc, sS[v][1], cd);
            cpw += sS[v][2];
#pragma unroll
            for (int i = 0; i < C; i++) cr[i] = fmaf(Tc, sS[v][3 + i], cr[i]);
            Tc *= sS[v][0];
        }
        tot += sS[v][2];
    }
    int stop = INT_MAX;
    float Ta[4];
#pragma unroll
    for (int r = 3; r >= 0; r--) {
        Tb[r] *= Tc;
        Ta[r] = Tb[r] * om[r];
        const uint64_t m = __ballot(Ta[r] <= T_thr);
        if (m) stop = base + r * 64 + __builtin_ctzll(m);
    }
    if (lane == 0) sStop[wv] = stop;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < CF_WPB; v++) stop = min(stop, sStop[v]);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int pos = base + r * 64 + lane;  // (the row body of composite_bw_block, kept in step by hand: see there)
        const bool inc = pos <= stop;
        const float w = inc ? a[r] * Tb[r] : 0.f;
        if constexpr (!DSIG) {
            if (base + r * 64 < N) {
#pragma unroll
                for (int i = 0; i < C; i++) buf_store(r_gr, (uint32_t)pos * (4u * C) + 4u * i, dR[i] * w);
            }
            continue;
        }
        float run_d = w * tt[r], run_r[C];
#pragma unroll
        for (int i = 0; i < C; i++) run_r[i] = w * rr[r][i];
        if constexpr (C == 3) {
            wave_incl_sum4(run_d, run_r[0], run_r[1], run_r[2]);
        } else {
            run_d = wave_incl_sum_dpp(run_d);
#pragma unroll
            for (int i = 0; i < C; i++) run_r[i] = wave_incl_sum_dpp(run_r[i]);
        }
        run_d += cd;
#pragma unroll
        for (int i = 0; i < C; i++) run_r[i] += cr[i];
        const float run_pw = DWS ? cpw + wave_incl_sum_dpp(pw[r]) : 0.f;
        float gs = gO + dD * (tt[r] * Ta[r] - (D - run_d)) + Ta[r] * dws[r] - (tot - run_pw);
        const bool live_row = base + r * 64 < N;
#pragma unroll
        for (int i = 0; i < C; i++) {
            gs += dR[i] * (rr[r][i] * Ta[r] - (RE[i] - run_r[i]));
            if (live_row) buf_store(r_gr, (uint32_t)pos * (4u * C) + 4u * i, dR[i] * w);
        }
        if (live_row) buf_store(r_gs, (uint32_t)pos * 4u, inc ? gs * dl[r] : 0.f);
        cd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run_d), 63));
        if (DWS) cpw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run_pw), 63));
#pragma unroll
        for (int i = 0; i < C; i++) cr[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run_r[i]), 63));
    }
}

// (composite_bw_kernel<3, false> takes 80 VGPRs: 6 waves/SIMD.  Measured with forced 7 / 8 waves per
// SIMD (tools/composite_bw_probe.py, 8192 marched rays): 9.9-10.0 / 10.3-10.5 us against 9.6 -
// spills.)  DWS: a non-NULL dL_dws.
template <int C, bool DWS>
__global__ __launch_bounds__(64 * CF_WPB) void composite_bw_kernel(
    const float* __restrict__ dL_dopacity, const float* __restrict__ dL_ddepth, const float* __restrict__ dL_drend,
    const float* __restrict__ dL_dws, const float* __restrict__ sigmas, const float* __restrict__ raws,
    const float* __restrict__ ws, const float* __restrict__ deltas, const float* __restrict__ ts,
    const int64_t* __restrict__ rays_a, int64_t R, const float* __restrict__ opacity,
    const float* __restrict__ depth, const float* __restrict__ rend, float T_thr, float* __restrict__ dL_dsigmas,
    float* __restrict__ dL_draws, float bg, int n_coop) {
    if ((int)blockIdx.x < n_coop) {
        for (int64_t row = blockIdx.x; cf_long_row(rays_a, R, row); row += n_coop)
            composite_bw_coop<C, DWS>(dL_dopacity, dL_ddepth, dL_drend, dL_dws, sigmas, raws, ws, deltas, ts, rays_a,
                                      row, opacity, depth, rend, T_thr, dL_dsigmas, dL_draws, bg);
        return;
    }
    bool taken;
    const RaySeg g = cf_own_ray(rays_a, R, n_coop, taken);
    if (taken) return;
    composite_bw_ray<C, DWS>(dL_dopacity, dL_ddepth, dL_drend, dL_dws, sigmas, raws, ws, deltas, ts, g, opacity, depth,
                             rend, T_thr, dL_dsigmas, dL_draws, bg);
}

}  // namespace ncn
