// Test rendering: the serial compositor of alive rays, the compaction of the test marcher's output
// and the device-driven test loop.
#pragma once
#include "workgroup.h"

namespace ncn {

// composite_test_multi_fw (volumerendering.cu:504-550): lane per alive ray, serial (test path).
// offsets (ncn_composite_test_fw_compact): NULL, or the start of ray n's samples in compacted
// sigmas / raws (ncn_test_compact); deltas / ts stay in the marcher's (alive, NS) layout.
__global__ __launch_bounds__(256) void composite_test_kernel(const float* __restrict__ sigmas,
                                                             const float* __restrict__ raws,
                                                             const float* __restrict__ deltas,
                                                             const float* __restrict__ ts, int64_t* __restrict__ alive,
                                                             int64_t A, int NS, int C, float T_thr,
                                                             const int32_t* __restrict__ n_eff,
                                                             float* __restrict__ opacity, float* __restrict__ depth,
                                                             float* __restrict__ rend,
                                                             const int32_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ ctrl) {
    if (ctrl) {
        A = ctrl[0];
        NS = ctrl[1];
    }
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= A) return;
    if (n_eff[n] == 0) {
        alive[n] = -1;
        return;
    }
    const int64_t r = alive[n];
    const int64_t base = offsets ? (int64_t)offsets[n] : n * (int64_t)NS;
    float T = 1.0f - opacity[r];
    for (int s = 0; s < n_eff[n]; s++) {
        const int64_t k = n * (int64_t)NS + s, kc = base + s;
        const float a = 1.0f - __expf(-sigmas[kc] * deltas[k]);
        const float w = a * T;
        for (int i = 0; i < C; i++) rend[r * C + i] = fmaf(w, raws[kc * C + i], rend[r * C + i]);
        depth[r] = fmaf(w, ts[k], depth[r]);
        opacity[r] += w;
        T *= 1.0f - a;
        if (T <= T_thr) {
            alive[n] = -1;
            break;
        }
    }
}

// Compaction of the test marcher's output (the fused test-render iteration): the valid samples of
// every alive ray (its first n_eff of NS slots) copied to consecutive rows of xyz_c / dir_c, ray n's
// rows starting at offsets[n]; count[0] = the total.  A workgroup scans its 256 rays' n_eff and
// reserves its rows with one atomic on count, so the workgroups' order in the output is arbitrary
// (the compositor reads through offsets; the field's arithmetic is per sample).  count must be 0.
__global__ __launch_bounds__(256) void test_compact_kernel(const float* __restrict__ xyzs,
                                                           const float* __restrict__ dirs,
                                                           const int32_t* __restrict__ n_eff, int64_t A, int NS,
                                                           int32_t* __restrict__ offsets, float* __restrict__ xyz_c,
                                                           float* __restrict__ dir_c, int32_t* __restrict__ count) {
    __shared__ int wsum[4];
    __shared__ int base;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = n < A ? n_eff[n] : 0;
    int tot;
    const int excl = block_excl_scan<256>(c, tot, wsum);
    if (threadIdx.x == 0) base = tot ? atomicAdd(count, tot) : 0;
    __syncthreads();
    const int off = base + excl;
    if (n >= A) return;
    offsets[n] = off;
    const float* X = xyzs + n * (int64_t)NS * 3;
    const float* D = dirs + n * (int64_t)NS * 3;
    for (int s = 0; s < c; s++) {
        const int64_t o = (int64_t)(off + s) * 3;
        xyz_c[o] = X[3 * s]; xyz_c[o + 1] = X[3 * s + 1]; xyz_c[o + 2] = X[3 * s + 2];
        dir_c[o] = D[3 * s]; dir_c[o + 1] = D[3 * s + 1]; dir_c[o + 2] = D[3 * s + 2];
    }
}

// Device-driven test loop (rendering.py:68-105 without a host read per iteration): ctrl (int32) =
// {0 alive rays A, 1 samples per ray NS, 2 samples so far, 3 done, 4 valid samples of the iteration,
//  5 next alive count, 6 iterations run, 7 alive x NS summed}.  After the compositor: the rays it
// kept (alive >= 0) are compacted into alive_next (order irrelevant: every ray is independent) and
// one thread forms the next iteration exactly as the reference's loop head does — stop when no ray
// is alive or samples >= max_samples, else NS = max(min(n_rays / A, 64), min_samples).  A done loop
// has A = 0, so further iterations launch empty.
// Block-range compaction for the device test loop: workgroup b owns a contiguous range of the
// A items (a multiple of 256 long), counts its output, reserves it with ONE atomic on the counter
// (a few hundred arrivals instead of one per 256 items: same-address atomics serialise at the
// memory side), then writes its items in order with a running offset.
constexpr int TL_BLOCKS = 256;
// The valid slots of the iteration as a list of (alive, NS)-layout indices (ray n's first n_eff[n]
// slots), count into ctrl[4].  The field evaluates x[idx[p]] for p < count and writes its outputs at
// idx[p] (its `order` operand), so nothing is copied.
__global__ __launch_bounds__(256) void test_index_kernel(const int32_t* __restrict__ n_eff, int32_t* __restrict__ ctrl,
                                                         int32_t* __restrict__ idx) {
    const int64_t A = ctrl[0];
    const int NS = ctrl[1];
    const int64_t per = ((A + TL_BLOCKS - 1) / TL_BLOCKS + 255) & ~(int64_t)255;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = min(A, lo + per);
    if (lo >= hi) return;  // (uniform)
    __shared__ int wsum[4];
    __shared__ int base;
    int cnt = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) cnt += n_eff[i];
    const int total = block_sum<256>(cnt, wsum);
    if (threadIdx.x == 0) base = total ? atomicAdd(ctrl + 4, total) : 0;
    __syncthreads();
    int run = base;
    for (int64_t c0 = lo; c0 < hi; c0 += 256) {
        const int64_t n = c0 + threadIdx.x;
        const int c = n < hi ? n_eff[n] : 0;
        const int off = block_excl_sweep<256>(c, run, wsum);
        const int first = (int)(n * NS);
        for (int s = 0; s < c; s++) idx[off + s] = first + s;
    }
}
// After the compositor: the rays it kept (alive >= 0) compacted into alive_next (order irrelevant:
// every ray is independent), their count into ctrl[5].
__global__ __launch_bounds__(256) void test_alive_compact_kernel(const int64_t* __restrict__ alive,
                                                                 int64_t* __restrict__ alive_next,
                                                                 int32_t* __restrict__ ctrl) {
    const int64_t A = ctrl[0];
    const int64_t per = ((A + TL_BLOCKS - 1) / TL_BLOCKS + 255) & ~(int64_t)255;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = min(A, lo + per);
    if (lo >= hi) return;  // (uniform)
    __shared__ int wsum[4];
    __shared__ int base;
    int cnt = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) cnt += alive[i] >= 0;
    const int total = block_sum<256>(cnt, wsum);
    if (threadIdx.x == 0) base = total ? atomicAdd(ctrl + 5, total) : 0;
    __syncthreads();
    int run = base;
    for (int64_t c0 = lo; c0 < hi; c0 += 256) {
        const int64_t n = c0 + threadIdx.x;
        const int64_t r = n < hi ? alive[n] : -1;
        const int off = block_excl_sweep<256>((int)(r >= 0), run, wsum);
        if (r >= 0) alive_next[off] = r;
    }
}
__global__ void test_loop_next_kernel(int32_t* __restrict__ ctrl, int64_t* __restrict__ total, int n_rays,
                                      int max_samples, int min_samples) {
    if (threadIdx.x != 0 || ctrl[3]) return;
    total[0] += ctrl[4];
    ctrl[6] += 1;
    ctrl[7] += ctrl[0] * ctrl[1];
    const int na = ctrl[5];
    ctrl[4] = 0;
    ctrl[5] = 0;
    const int samples = ctrl[2];
    if (na == 0 || samples >= max_samples) {
        ctrl[3] = 1;
        ctrl[0] = 0;
        return;
    }
    const int ns = max(min(n_rays / na, 64), min_samples);
    ctrl[0] = na;
    ctrl[1] = ns;
    ctrl[2] = samples + ns;
}

}  // namespace ncn
