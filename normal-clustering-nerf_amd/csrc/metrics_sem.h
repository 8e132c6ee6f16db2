// The semantic metrics for metrics.hip: one view's (n_pix, K) logits into the K x K confusion matrix of
// the reference's SemanticMetrics (argmax, mask, confusion_matrix: four passes and a host read there)
// in ONE streaming launch, and the scores of its compute() by one workgroup.
//
// The rows are `row_stride` floats apart (the renderer's `sem` is a channel slice of a wider buffer),
// so a thread that walked its own pixel's row would make every wave load touch 64 cache lines.  A
// workgroup instead stages a tile of SEM_ROWS rows in LDS: element e of the tile is
// (row e / K, channel e % K), consecutive lanes take consecutive e, so a wave reads contiguous spans of
// K floats and never what lies between the rows.  The tile's row stride in LDS is K | 1, odd, so the
// second phase — thread t < SEM_ROWS takes row t — reads 32 different banks per half-wave (ds_read_b32
// banks are dword address mod 32).  Counting goes to K * K LDS counters with LDS atomics; they are
// flushed once per workgroup with 64-bit integer atomics (exact and order free, as metrics_select.h's
// histograms).  128 rows and not 256: at K = 40 a workgroup then holds 27 KiB of LDS and all 1024
// workgroups of the grid are resident at once; measured 57 against 66 us.
#pragma once
#include "workgroup.h"

namespace ncn {

constexpr int SEM_THREADS = 256;
constexpr int SEM_ROWS = 128;            // rows of a tile; K = 64: 48.5 KiB of LDS with the counters
constexpr int SEM_MAX_CLS = 64;          // NCN_SEM_MAX_CLASSES
constexpr int SEM_UNROLL = 8;            // LDS reads of the argmax loop that issue together
constexpr int SEM_LOADS = 8;             // global loads a thread has in flight while staging

// the counters (K * K and the two totals) and the tile at row stride K | 1
static inline int sem_lds_words(int K) { return K * K + 2 + SEM_ROWS * (K | 1); }
static_assert(4 * (SEM_MAX_CLS * SEM_MAX_CLS + 2 + SEM_ROWS * (SEM_MAX_CLS | 1)) <= 64 * 1024, "the tile fits 64 KiB");

// torch.argmax's order on one row: b replaces a if it is greater, or the first NaN
__device__ __forceinline__ bool sem_beats(float b, float a) { return b > a || (b != b && a == a); }

__global__ __launch_bounds__(SEM_THREADS) void sem_confusion_kernel(
    const float* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ labels, int64_t label_shift,
    int64_t ignore_label, int64_t n_pix, int K, int64_t* __restrict__ conf, int64_t* __restrict__ counts,
    int32_t* __restrict__ pred_labels) {
    extern __shared__ uint32_t sem_lds[];
    const int t = threadIdx.x, KK = K * K, ls = K | 1;
    uint32_t* h = sem_lds;  // [KK] the matrix, [KK] counted, [KK + 1] out of range
    float* tile = reinterpret_cast<float*>(sem_lds + KK + 2);
    for (int b = t; b < KK + 2; b += SEM_THREADS) h[b] = 0u;
    // element t of a tile and the step to element t + SEM_THREADS, as (row, channel)
    const int row0 = t / K, col0 = t - row0 * K, drow = SEM_THREADS / K, dcol = SEM_THREADS - drow * K;
    uint32_t n_ok = 0u, n_out = 0u;
    const int64_t n_tiles = (n_pix + SEM_ROWS - 1) / SEM_ROWS;
    for (int64_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const int64_t base = ti * SEM_ROWS;
        const int rows = (int)(n_pix - base < SEM_ROWS ? n_pix - base : SEM_ROWS);
        // ---- stage rows [base, base + rows) ----
        const float* src = logits + base * row_stride;
        int row = row0, col = col0;
        while (row < rows) {
            float v[SEM_LOADS];
            int at[SEM_LOADS];
#pragma unroll
            for (int u = 0; u < SEM_LOADS; u++) {
                at[u] = row < rows ? row * ls + col : -1;
                v[u] = at[u] >= 0 ? src[(int64_t)row * row_stride + col] : 0.0f;
                col += dcol;
                row += drow;
                if (col >= K) {
                    col -= K;
                    row++;
                }
            }
#pragma unroll
            for (int u = 0; u < SEM_LOADS; u++) {
                if (at[u] >= 0) tile[at[u]] = v[u];
            }
        }
        __syncthreads();  // (the first one also covers the zeroed counters)
        // ---- thread t: pixel base + t ----
        if (t < rows) {
            const int64_t i = base + t;
            const int64_t lab = labels[i] + label_shift;
            const float* r = tile + t * ls;
            float best = r[0];
            int p = 0, c = 1;
            for (; c + SEM_UNROLL <= K; c += SEM_UNROLL) {  // the LDS reads of a group issue together
                float x[SEM_UNROLL];
#pragma unroll
                for (int u = 0; u < SEM_UNROLL; u++) x[u] = r[c + u];
#pragma unroll
                for (int u = 0; u < SEM_UNROLL; u++) {
                    if (sem_beats(x[u], best)) {
                        best = x[u];
                        p = c + u;
                    }
                }
            }
            for (; c < K; c++) {
                const float x = r[c];
                if (sem_beats(x, best)) {
                    best = x;
                    p = c;
                }
            }
            if (lab != ignore_label) {
                if (lab >= 0 && lab < K) {
                    atomicAdd(&h[(int)lab * K + p], 1u);
                    n_ok++;
                } else {
                    n_out++;
                }
            }
            if (pred_labels != nullptr) pred_labels[i] = p;
        }
        __syncthreads();  // the tile is rewritten
    }
    n_ok = wave_sum(n_ok);
    n_out = wave_sum(n_out);
    if ((t & (WAVE - 1)) == 0) {
        if (n_ok != 0u) atomicAdd(&h[KK], n_ok);
        if (n_out != 0u) atomicAdd(&h[KK + 1], n_out);
    }
    __syncthreads();
    for (int b = t; b < KK + 2; b += SEM_THREADS) {
        if (h[b] == 0u) continue;
        int64_t* dst = b < KK ? conf + b : counts + (b - KK);
        atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)h[b]);
    }
}

// semantic_metrics.py:42-66 from the matrix; one wave, thread c takes class c.
__global__ __launch_bounds__(WAVE) void sem_finalise_kernel(const int64_t* __restrict__ conf, int K,
                                                            float* __restrict__ out) {
    __shared__ double iou[SEM_MAX_CLS], acc[SEM_MAX_CLS];
    __shared__ long long row_sum[SEM_MAX_CLS], diag[SEM_MAX_CLS];
    const int c = threadIdx.x;
    if (c < K) {
        long long r = 0, s = 0;
        for (int j = 0; j < K; j++) {
            r += conf[c * K + j];
            s += conf[j * K + c];
        }
        const long long d = conf[c * K + c];
        iou[c] = (double)d / (double)(r + s - d);  // 0 / 0: NaN
        acc[c] = (double)d / (double)r;
        row_sum[c] = r;
        diag[c] = d;
        out[4 + c] = (float)iou[c];
    }
    __syncthreads();
    if (c != 0) return;
    double iou_all = 0.0, iou_valid = 0.0, acc_valid = 0.0;
    long long n_all = 0, n_valid = 0, trace = 0, total = 0;
    for (int j = 0; j < K; j++) {
        if (iou[j] == iou[j]) {
            iou_all += iou[j];
            n_all++;
        }
        if (row_sum[j] > 0) {
            iou_valid += iou[j];
            acc_valid += acc[j];
            n_valid++;
        }
        trace += diag[j];
        total += row_sum[j];
    }
    out[0] = (float)(iou_all / (double)n_all);
    out[1] = (float)(iou_valid / (double)n_valid);
    out[2] = (float)((double)trace / (double)total);
    out[3] = (float)(acc_valid / (double)n_valid);
}

}  // namespace ncn
