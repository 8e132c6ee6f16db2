// Exact selection for metrics.hip: the k-th smallest (k = (n - 1) / 2, torch.median's lower middle)
// of the unmarked entries of an array of non-negative floats, n read on the device.
//
// A non-negative float's bit pattern orders as an unsigned integer, so the element is found by
// narrowing its key: three passes histogram the key bits 31..21, 20..10 and 9..0 (2048, 2048 and 1024
// bins) of the entries that match the prefix found so far.  A pass counts in LDS (8 KiB of counters
// per workgroup) and flushes its non-empty bins with integer atomics, which are exact and order
// free; the prefix is not stored anywhere: every workgroup re-derives it from the earlier passes'
// histograms (a 256-thread scan of at most 2048 counters from L2).  The host never reads n or k.
#pragma once
#include "workgroup.h"

namespace ncn {

constexpr uint32_t SEL_MARK = 0xFFFFFFFFu;
constexpr int SEL_THREADS = 256;
constexpr int SEL_PER_THREAD = 8;    // entries per thread before the grid stops growing
constexpr int SEL_MAX_BLOCKS = 512;
constexpr int SEL_MAX_BINS = 2048;
constexpr int SEL_WORDS = 2048 + 2048 + 1024;  // one array's three histograms

__device__ __forceinline__ int sel_bins(int pass) { return pass == 2 ? 1024 : 2048; }
__device__ __forceinline__ int sel_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__device__ __forceinline__ int sel_offset(int pass) { return pass * 2048; }

// The bin of `hist` (nbins counters) that holds the k-th entry (from 0) and k's rank inside that bin;
// false if the histogram holds k entries or fewer.  All SEL_THREADS threads call it; tmp: 8 ints of LDS.
__device__ __forceinline__ bool sel_find(const uint32_t* __restrict__ hist, int nbins, int k, int& bin, int& k_in,
                                         int* tmp) {
    const int t = threadIdx.x, lane = t & (WAVE - 1), per = nbins / SEL_THREADS;  // 8 or 4
    int c[SEL_MAX_BINS / SEL_THREADS], s = 0;
#pragma unroll
    for (int i = 0; i < SEL_MAX_BINS / SEL_THREADS; i++) {
        c[i] = i < per ? (int)hist[t * per + i] : 0;
        s += c[i];
    }
    int incl = wave_incl_sum(s, lane);
    __syncthreads();  // tmp may still be read from an earlier call
    if (lane == WAVE - 1) tmp[t / WAVE] = incl;
    if (t == 0) tmp[6] = 0;
    __syncthreads();
    for (int w = 0; w < t / WAVE; w++) incl += tmp[w];
    int excl = incl - s;
    if (s > 0 && k >= excl && k < incl) {  // exactly one thread
#pragma unroll
        for (int i = 0; i < SEL_MAX_BINS / SEL_THREADS; i++) {
            if (k >= excl && k < excl + c[i]) {
                tmp[4] = t * per + i;
                tmp[5] = k - excl;
                tmp[6] = 1;
            }
            excl += c[i];
        }
    }
    __syncthreads();
    bin = tmp[4];
    k_in = tmp[5];
    return tmp[6] != 0;
}

// The key prefix after `passes` passes and k's rank among the entries that share it.
__device__ __forceinline__ bool sel_prefix(const uint32_t* __restrict__ hist, int passes, int& k, uint32_t& prefix,
                                           int* tmp) {
    prefix = 0u;
    for (int p = 0; p < passes; p++) {
        int bin, k_in;
        if (!sel_find(hist + sel_offset(p), sel_bins(p), k, bin, k_in, tmp)) return false;
        prefix |= (uint32_t)bin << sel_shift(p);
        k = k_in;
    }
    return true;
}

__global__ void select_zero_kernel(uint32_t* __restrict__ ws, int total) {
    const int i = blockIdx.x * SEL_THREADS + threadIdx.x;
    if (i < total) ws[i] = 0u;
}

__global__ __launch_bounds__(SEL_THREADS) void select_hist_kernel(const float* __restrict__ vals, int64_t capacity,
                                                                  const int64_t* __restrict__ n_dev,
                                                                  uint32_t* __restrict__ ws, int pass) {
    __shared__ uint32_t h[SEL_MAX_BINS];
    __shared__ int tmp[8];
    const int t = threadIdx.x;
    const int64_t n = n_dev[0];
    if (n <= 0 || n > capacity) return;  // the same in every thread
    const uint32_t* v = reinterpret_cast<const uint32_t*>(vals) + (int64_t)blockIdx.y * capacity;
    uint32_t* hist = ws + (int64_t)blockIdx.y * SEL_WORDS;
    int k = (int)((n - 1) / 2);
    uint32_t prefix;
    if (!sel_prefix(hist, pass, k, prefix, tmp)) return;  // the same in every thread
    const int shift = sel_shift(pass), nbins = sel_bins(pass);
    const uint32_t above = pass == 0 ? 0u : ~((1u << sel_shift(pass - 1)) - 1u);  // the bits the earlier passes fixed
    for (int b = t; b < nbins; b += SEL_THREADS) h[b] = 0u;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * SEL_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SEL_THREADS + t; i < capacity; i += stride) {
        const uint32_t key = v[i];
        if (key != SEL_MARK && (key & above) == prefix) atomicAdd(&h[(key >> shift) & (uint32_t)(nbins - 1)], 1u);
    }
    __syncthreads();
    uint32_t* out = hist + sel_offset(pass);
    for (int b = t; b < nbins; b += SEL_THREADS) {
        if (h[b] != 0u) atomicAdd(&out[b], h[b]);
    }
}

__global__ __launch_bounds__(SEL_THREADS) void select_pick_kernel(int64_t capacity, const int64_t* __restrict__ n_dev,
                                                                  const uint32_t* __restrict__ ws,
                                                                  float* __restrict__ out) {
    __shared__ int tmp[8];
    const int64_t n = n_dev[0];
    uint32_t key = 0x7FC00000u;  // NaN: no such element
    if (n > 0 && n <= capacity) {
        int k = (int)((n - 1) / 2);
        uint32_t prefix;
        if (sel_prefix(ws + (int64_t)blockIdx.x * SEL_WORDS, 3, k, prefix, tmp)) key = prefix;
    }
    if (threadIdx.x == 0) out[blockIdx.x] = __uint_as_float(key);
}

}  // namespace ncn
