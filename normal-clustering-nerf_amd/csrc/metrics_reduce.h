// Fixed-order workgroup reductions of the metric kernels (metrics.hip): xor-shuffles inside each
// wave, then the waves' totals in wave order.  Every thread of the workgroup must call them.
#pragma once
#include "common.h"

namespace ncn {

// torch's min / max: a NaN wins
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || b != b) ? a + b : fminf(a, b); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }

// v[k] <- the workgroup's total of v[k], in every thread.  red: [THREADS / 64][K] doubles of LDS.
template <int K, int THREADS>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*red)[K]) {
    constexpr int NW = THREADS / WAVE;
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, WAVE);
    }
    __syncthreads();  // red may still be read from an earlier call
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[threadIdx.x / WAVE][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double t = red[0][k];
#pragma unroll
        for (int w = 1; w < NW; w++) t += red[w][k];
        v[k] = t;
    }
}

// (lo, hi) <- the workgroup's NaN-propagating min and max.  red: [THREADS / 64][2] floats of LDS.
template <int THREADS>
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float (*red)[2]) {
    constexpr int NW = THREADS / WAVE;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = nan_min(lo, __shfl_xor(lo, off, WAVE));
        hi = nan_max(hi, __shfl_xor(hi, off, WAVE));
    }
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        red[threadIdx.x / WAVE][0] = lo;
        red[threadIdx.x / WAVE][1] = hi;
    }
    __syncthreads();
    lo = red[0][0];
    hi = red[0][1];
#pragma unroll
    for (int w = 1; w < NW; w++) {
        lo = nan_min(lo, red[w][0]);
        hi = nan_max(hi, red[w][1]);
    }
}

}  // namespace ncn
