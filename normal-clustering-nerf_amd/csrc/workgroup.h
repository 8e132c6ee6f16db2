// Wave and workgroup sums, scans and the last-workgroup hand-off: the one statement of these
// primitives (the DPP scans and permlane multi-sums of common.h are a different design).
//
// Contract of every block_* function:
//  * every thread of the workgroup calls it (it holds a barrier), THREADS is a multiple of 64 and
//    equals blockDim.x;
//  * the order is fixed: per wave an xor-butterfly (sums) or a Hillis-Steele scan, lane 0 (63) of each
//    wave to LDS, then the waves' values left to right, red[0] + red[1] + ..., in every thread.  Two
//    launches with the same input give the same bits;
//  * the LDS array is read by every thread until it returns, so the CALLER owns the barrier that
//    guards its reuse: a __syncthreads() before the same array is passed to a second call or written
//    otherwise.  (block_excl_sweep, made for loops, ends with that barrier itself.)
#pragma once
#include "common.h"

namespace ncn {

// ---- wave level (float, double, int, 64-bit integers: HIP splits 8-byte values into two shuffles) ----
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// Inclusive scan across the 64 lanes (Hillis-Steele, 6 steps).
template <typename T>
__device__ __forceinline__ T wave_incl_sum(T v, int lane) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const T o = __shfl_up(v, off, WAVE);
        if (lane >= off) v += o;
    }
    return v;
}

// torch's min / max: a NaN wins
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || b != b) ? a + b : fminf(a, b); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }

// ---- workgroup reduction ----
// v[k] <- op(k, ., .) folded over the workgroup's v[k], in every thread.  red: [THREADS / 64][K] of LDS.
template <int K, int THREADS, typename T, typename Op>
__device__ __forceinline__ void block_reduce(T (&v)[K], T (*red)[K], Op op) {
    static_assert(THREADS % WAVE == 0, "whole waves");
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] = op(k, v[k], __shfl_xor(v[k], off, WAVE));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[threadIdx.x / WAVE][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        T t = red[0][k];
#pragma unroll
        for (int w = 1; w < THREADS / WAVE; w++) t = op(k, t, red[w][k]);
        v[k] = t;
    }
}

template <int K, int THREADS, typename T>
__device__ __forceinline__ void block_sum(T (&v)[K], T (*red)[K]) {
    block_reduce<K, THREADS>(v, red, [](int, T a, T b) { return a + b; });
}
// one value; red: THREADS / 64 words of LDS
template <int THREADS, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    T a[1] = {v};
    block_sum<1, THREADS>(a, reinterpret_cast<T(*)[1]>(red));
    return a[0];
}

// (lo, hi) <- the workgroup's NaN-propagating min and max.  red: [THREADS / 64][2] floats of LDS.
template <int THREADS>
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float (*red)[2]) {
    float v[2] = {lo, hi};
    block_reduce<2, THREADS>(v, red, [](int k, float a, float b) { return k == 0 ? nan_min(a, b) : nan_max(a, b); });
    lo = v[0];
    hi = v[1];
}

// ---- workgroup exclusive scan (int, long long) ----
// Returns the sum of v over the threads in front of this one; total <- the workgroup's sum.
// wave_tot: THREADS / 64 words of LDS.
template <int THREADS, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T& total, T* wave_tot) {
    static_assert(THREADS % WAVE == 0, "whole waves");
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const T incl = wave_incl_sum(v, lane);
    if (lane == WAVE - 1) wave_tot[wave] = incl;
    __syncthreads();
    T before = incl - v, all = 0;
#pragma unroll
    for (int w = 0; w < THREADS / WAVE; w++) {
        if (w < wave) before += wave_tot[w];
        all += wave_tot[w];
    }
    total = all;
    return before;
}
// The sweep form, for a loop over chunks of THREADS values: the prefix continues from carry, which
// then takes the chunk's sum (every thread keeps the same carry).  Ends with the barrier that lets
// the next sweep rewrite wave_tot.
template <int THREADS, typename T>
__device__ __forceinline__ T block_excl_sweep(T v, T& carry, T* wave_tot) {
    T total;
    const T before = carry + block_excl_scan<THREADS>(v, total, wave_tot);
    carry += total;
    __syncthreads();
    return before;
}

// ---- last-workgroup hand-off ----
// Thread 0 publishes the workgroup's partial v to *slot and adds one arrival; true, in every
// thread, in the workgroup that arrived last (it then reads the slots with agent-scope loads and
// resets *arrive).  This is the sc1 form of MI355X_MICROARCH.md "Correctness boundaries"
// (inter-workgroup visibility): the partial is stored with an agent-scope (sc1) store and drained
// (vmcnt(0)) before the arrival add, and the last workgroup reads the partials with agent-scope
// (sc1) loads.  It relies on gfx9's in-order completion of one wave's vector memory operations
// after vmcnt(0), not on a HIP release/acquire pair: an agent-scope release fence writes back the
// whole L2 (buffer_wbl2), which right after the table-gradient scatter measured ~40 us.  (The asm's
// "memory" clobber keeps the compiler from moving the store past the add.)
template <typename T>
__device__ __forceinline__ bool last_block_arrive(T* slot, T v, unsigned* arrive) {
    __shared__ bool last;
    if (threadIdx.x == 0) {
        __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    return last;
}

// total_samples.sum() by one 1024-thread workgroup (+ optional f64 accumulators: acc[0] +=
// counter[0] (marched), acc[1] += the sum (composited)) — ncn_count_samples, and the extra
// workgroup of ncn_photo_normals_count_fwd.
constexpr int CS_THREADS = 1024;
__device__ __forceinline__ void count_samples_wg(const int64_t* __restrict__ total, int64_t R,
                                                 const int32_t* __restrict__ counter, int64_t* __restrict__ sum_out,
                                                 double* __restrict__ acc) {
    __shared__ long long part[CS_THREADS / WAVE];
    long long v = 0;
    for (int64_t i = threadIdx.x; i < R; i += CS_THREADS) v += total[i];
    const long long t = block_sum<CS_THREADS>(v, part);
    if (threadIdx.x == 0) {
        *sum_out = t;
        if (acc) {
            acc[0] += counter ? (double)counter[0] : 0.0;
            acc[1] += (double)t;
        }
    }
}

}  // namespace ncn
