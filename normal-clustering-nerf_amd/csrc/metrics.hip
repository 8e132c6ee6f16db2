// Validation metrics for gfx950: the per-view quantities of the reference's NeRFMTMetricsPerIm
// (metrics/metrics.py) — PSNR, three SSIMs, masked depth errors, angular errors of the normals and
// their exact medians — behind the C ABI of include/ncnerf_metrics.h.
//  * metrics_ssim.h    the LDS-tiled SSIM pass (both Gaussian SSIMs and the 7x7 one in one launch)
//  * metrics_select.h  exact k-th smallest by three histogram passes
//  * metrics_sem.h     the semantic confusion matrix of a view in one launch, and its scores
//                      (include/ncnerf_sem.h)
// Every sum has a fixed order: per thread, xor-shuffles per wave, the waves' totals in wave order,
// the workgroups' partial sums by ONE workgroup (thread t takes partials t, t + 256, ...).  Partial
// sums are doubles, so the order is also irrelevant to well below an f32 ulp.  No float atomics.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include "workgroup.h"
#include "metrics_ssim.h"
#include "metrics_select.h"
#include "metrics_sem.h"
#include "../../include/ncnerf_metrics.h"
#include "../../include/ncnerf_sem.h"

namespace ncn {

constexpr int MT_THREADS = 256;      // the streaming passes and every final reduction
constexpr int MT_MAX_BLOCKS = 1024;  // P(n) of ncnerf_metrics.h

static inline int stream_blocks(int64_t n) { return (int)std::min<int64_t>(cdiv(n, MT_THREADS), MT_MAX_BLOCKS); }

// ---- pointwise errors ----
// One thread per pixel, grid-stride.  partials[b] = (rgb sq, depth sq, depth abs, depth count, gt min,
// gt max) of workgroup b.
__global__ __launch_bounds__(MT_THREADS) void pointwise_kernel(const float* __restrict__ rgb_p,
                                                               const float* __restrict__ rgb_t,
                                                               const float* __restrict__ dep_p,
                                                               const float* __restrict__ dep_t, int64_t n_pix,
                                                               double* __restrict__ partials) {
    __shared__ double red[MT_THREADS / WAVE][4];
    __shared__ float redm[MT_THREADS / WAVE][2];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    float lo = INFINITY, hi = -INFINITY;
    const int64_t stride = (int64_t)gridDim.x * MT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; i < n_pix; i += stride) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float t = rgb_t[3 * i + c], d = rgb_p[3 * i + c] - t;
            s[0] += (double)(d * d);
            lo = nan_min(lo, t);
            hi = nan_max(hi, t);
        }
        if (dep_t != nullptr) {
            const float t = dep_t[i];
            if (t > 0.0f) {
                const float d = dep_p[i] - t;
                s[1] += (double)(d * d);
                s[2] += (double)fabsf(d);
                s[3] += 1.0;
            }
        }
    }
    block_sum<4, MT_THREADS>(s, red);
    block_minmax<MT_THREADS>(lo, hi, redm);
    if (threadIdx.x == 0) {
        double* o = partials + 6 * (int64_t)blockIdx.x;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
        o[4] = (double)lo; o[5] = (double)hi;
    }
}

__global__ __launch_bounds__(MT_THREADS) void pointwise_reduce_kernel(const double* __restrict__ partials, int nb,
                                                                      double* __restrict__ sums,
                                                                      int64_t* __restrict__ depth_count,
                                                                      float* __restrict__ range) {
    __shared__ double red[MT_THREADS / WAVE][4];
    __shared__ float redm[MT_THREADS / WAVE][2];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    float lo = INFINITY, hi = -INFINITY;
    for (int b = threadIdx.x; b < nb; b += MT_THREADS) {
        const double* p = partials + 6 * (int64_t)b;
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; s[3] += p[3];
        lo = nan_min(lo, (float)p[4]);
        hi = nan_max(hi, (float)p[5]);
    }
    block_sum<4, MT_THREADS>(s, red);
    block_minmax<MT_THREADS>(lo, hi, redm);
    if (threadIdx.x == 0) {
        sums[0] = s[0]; sums[1] = s[1]; sums[2] = s[2];
        depth_count[0] = (int64_t)s[3];
        range[0] = lo; range[1] = hi;
    }
}

// ---- angles ----
// normals_metrics.py:_angular_errors in f32, operation for operation: x / (|x| + 1e-8), the three
// products summed left to right, clamp (NaN kept), acos, * (float)(180 / pi).  The flipped
// prediction's dot product is the exact negative.
constexpr uint32_t ANGLE_MARK = 0xFFFFFFFFu;
constexpr uint32_t ANGLE_NAN = 0x7FC00000u;

__device__ __forceinline__ float clamp_unit(float d) { return d < -1.0f ? -1.0f : (d > 1.0f ? 1.0f : d); }

__global__ __launch_bounds__(MT_THREADS) void angles_kernel(const float* __restrict__ np, const float* __restrict__ nt,
                                                            int64_t n_pix, float* __restrict__ angles,
                                                            double* __restrict__ partials) {
    __shared__ double red[MT_THREADS / WAVE][4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};  // angle sum, min-angle sum, valid, NaN
    const float rad_to_deg = (float)(180.0 / M_PI);
    const int64_t stride = (int64_t)gridDim.x * MT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; i < n_pix; i += stride) {
        const float t0 = nt[3 * i], t1 = nt[3 * i + 1], t2 = nt[3 * i + 2];
        uint32_t ka = ANGLE_MARK, km = ANGLE_MARK;
        if (fabsf(t0) + fabsf(t1) + fabsf(t2) > 0.0f) {
            const float p0 = np[3 * i], p1 = np[3 * i + 1], p2 = np[3 * i + 2];
            const float pn = sqrtf(p0 * p0 + p1 * p1 + p2 * p2) + 1e-8f;
            const float tn = sqrtf(t0 * t0 + t1 * t1 + t2 * t2) + 1e-8f;
            const float dot = (p0 / pn) * (t0 / tn) + (p1 / pn) * (t1 / tn) + (p2 / pn) * (t2 / tn);
            const float a = acosf(clamp_unit(dot)) * rad_to_deg;
            const float f = acosf(clamp_unit(-dot)) * rad_to_deg;
            const bool bad = a != a || f != f;
            const float m = bad ? a + f : (f < a ? f : a);
            s[0] += (double)a;
            s[1] += (double)m;
            s[2] += 1.0;
            s[3] += bad ? 1.0 : 0.0;
            ka = a != a ? ANGLE_NAN : __float_as_uint(a);
            km = m != m ? ANGLE_NAN : __float_as_uint(m);
        }
        angles[i] = __uint_as_float(ka);
        angles[n_pix + i] = __uint_as_float(km);
    }
    block_sum<4, MT_THREADS>(s, red);
    if (threadIdx.x == 0) {
        double* o = partials + 4 * (int64_t)blockIdx.x;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
    }
}

__global__ __launch_bounds__(MT_THREADS) void angles_reduce_kernel(const double* __restrict__ partials, int nb,
                                                                   double* __restrict__ sums,
                                                                   int64_t* __restrict__ counts) {
    __shared__ double red[MT_THREADS / WAVE][4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += MT_THREADS) {
        const double* p = partials + 4 * (int64_t)b;
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; s[3] += p[3];
    }
    block_sum<4, MT_THREADS>(s, red);
    if (threadIdx.x == 0) {
        sums[0] = s[0]; sums[1] = s[1];
        counts[0] = (int64_t)s[2]; counts[1] = (int64_t)s[3];
    }
}

// ---- the SSIM means from the tiles' partial sums ----
__global__ __launch_bounds__(MT_THREADS) void ssim_reduce_kernel(const double* __restrict__ partials, int nb, int H,
                                                                 int W, float* __restrict__ ssim) {
    __shared__ double red[MT_THREADS / WAVE][3];
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += MT_THREADS) {
        const double* p = partials + 3 * (int64_t)b;
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
    }
    block_sum<3, MT_THREADS>(s, red);
    if (threadIdx.x == 0) {
        const double ng = 3.0 * (double)(H - 2 * SS_R) * (double)(W - 2 * SS_R);
        const double nb7 = 3.0 * (double)(H - 2 * SS_RB) * (double)(W - 2 * SS_RB);
        ssim[0] = (float)(s[0] / ng);
        ssim[1] = (float)(s[1] / ng);
        ssim[2] = (float)(s[2] / nb7);
    }
}

// ---- the row ----
__global__ void finalise_kernel(const double* __restrict__ pw, const int64_t* __restrict__ dcount, int64_t n_rgb,
                                const float* __restrict__ ssim, const double* __restrict__ asum,
                                const int64_t* __restrict__ acount, const float* __restrict__ med,
                                float* __restrict__ row) {
    if (threadIdx.x != 0) return;
    const float qnan = __uint_as_float(ANGLE_NAN);
    row[0] = -10.0f * log10f((float)(pw[0] / (double)n_rgb));
    row[1] = ssim[0]; row[2] = ssim[1]; row[3] = ssim[2];
    const int64_t nd = dcount != nullptr ? dcount[0] : 0;
    row[4] = nd > 0 ? sqrtf((float)(pw[1] / (double)nd)) : 0.0f;
    row[5] = nd > 0 ? (float)(pw[2] / (double)nd) : 0.0f;
    row[6] = nd > 0 ? 1.0f : 0.0f;
    const int64_t nv = acount != nullptr ? acount[0] : 0;
    const bool bad = nv > 0 && acount[1] > 0;
    row[7] = nv > 0 ? (bad ? qnan : (float)(asum[0] / (double)nv)) : 0.0f;
    row[8] = nv > 0 ? (bad ? qnan : med[0]) : 0.0f;
    row[9] = nv > 0 ? (bad ? qnan : (float)(asum[1] / (double)nv)) : 0.0f;
    row[10] = nv > 0 ? (bad ? qnan : med[1]) : 0.0f;
    row[11] = nv > 0 ? 1.0f : 0.0f;
}

}  // namespace ncn

using namespace ncn;

extern "C" {

int ncn_metrics_pointwise(const float* rgb_pred, const float* rgb_gt, const float* depth_pred, const float* depth_gt,
                          int64_t n_pix, double* ws, int64_t ws_doubles, double* sums, int64_t* depth_count,
                          float* range, void* stream) {
    NCN_REQUIRE(n_pix >= 1 && rgb_pred != nullptr && rgb_gt != nullptr && sums != nullptr && depth_count != nullptr &&
                    range != nullptr,
                hipErrorInvalidValue, "ncn_metrics_pointwise: bad arguments (n_pix = %lld)", (long long)n_pix);
    NCN_REQUIRE((depth_pred == nullptr) == (depth_gt == nullptr), hipErrorInvalidValue,
                "ncn_metrics_pointwise: depth_pred and depth_gt go together");
    const int nb = stream_blocks(n_pix);
    NCN_REQUIRE(ws != nullptr && ws_doubles >= 6 * (int64_t)nb, hipErrorInvalidValue,
                "ncn_metrics_pointwise: workspace of %lld doubles, %lld needed", (long long)ws_doubles, 6LL * nb);
    hipLaunchKernelGGL(pointwise_kernel, dim3(nb), dim3(MT_THREADS), 0, (hipStream_t)stream, rgb_pred, rgb_gt,
                       depth_pred, depth_gt, n_pix, ws);
    NCN_LAUNCH_CHECK("ncn_metrics_pointwise");
    hipLaunchKernelGGL(pointwise_reduce_kernel, dim3(1), dim3(MT_THREADS), 0, (hipStream_t)stream, ws, nb, sums,
                       depth_count, range);
    NCN_LAUNCH_CHECK("ncn_metrics_pointwise (reduce)");
    return 0;
}

int ncn_metrics_ssim(const float* rgb_pred, const float* rgb_gt, int H, int W, const float* range, double* ws,
                     int64_t ws_doubles, float* maps, float* ssim, void* stream) {
    NCN_REQUIRE(rgb_pred != nullptr && rgb_gt != nullptr && range != nullptr && ssim != nullptr, hipErrorInvalidValue,
                "ncn_metrics_ssim: null argument");
    NCN_REQUIRE(H >= SS_TAPS && W >= SS_TAPS, hipErrorInvalidValue,
                "ncn_metrics_ssim: %dx%d image, the 11x11 window needs at least 11x11", H, W);
    const int64_t gx = cdiv(W, SS_TW), gy = cdiv(H, SS_TH);
    NCN_REQUIRE(gy <= 65535 && gx * gy <= 0x7FFFFFFF, hipErrorInvalidValue, "ncn_metrics_ssim: %dx%d is too large", H, W);
    NCN_REQUIRE(ws != nullptr && ws_doubles >= 3 * gx * gy, hipErrorInvalidValue,
                "ncn_metrics_ssim: workspace of %lld doubles, %lld needed", (long long)ws_doubles, (long long)(3 * gx * gy));
    SsimTaps taps = {NCN_SSIM_TAPS, 0.0f};
    double wsum = 0.0;  // of the 2-D window torchmetrics builds, g g^T in f32
    for (int i = 0; i < SS_TAPS; i++)
        for (int j = 0; j < SS_TAPS; j++) wsum += (double)(taps.g[abs(i - SS_R)] * taps.g[abs(j - SS_R)]);
    taps.eps = (float)(wsum - 1.0);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(SS_THREADS), 0, (hipStream_t)stream,
                       rgb_pred, rgb_gt, H, W, range, taps, ws, maps);
    NCN_LAUNCH_CHECK("ncn_metrics_ssim");
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(1), dim3(MT_THREADS), 0, (hipStream_t)stream, ws, (int)(gx * gy), H, W,
                       ssim);
    NCN_LAUNCH_CHECK("ncn_metrics_ssim (reduce)");
    return 0;
}

int ncn_metrics_angles(const float* normals_pred, const float* normals_gt, int64_t n_pix, float* angles, double* ws,
                       int64_t ws_doubles, double* sums, int64_t* counts, void* stream) {
    NCN_REQUIRE(n_pix >= 1 && normals_pred != nullptr && normals_gt != nullptr && angles != nullptr && sums != nullptr &&
                    counts != nullptr,
                hipErrorInvalidValue, "ncn_metrics_angles: bad arguments (n_pix = %lld)", (long long)n_pix);
    const int nb = stream_blocks(n_pix);
    NCN_REQUIRE(ws != nullptr && ws_doubles >= 4 * (int64_t)nb, hipErrorInvalidValue,
                "ncn_metrics_angles: workspace of %lld doubles, %lld needed", (long long)ws_doubles, 4LL * nb);
    hipLaunchKernelGGL(angles_kernel, dim3(nb), dim3(MT_THREADS), 0, (hipStream_t)stream, normals_pred, normals_gt, n_pix,
                       angles, ws);
    NCN_LAUNCH_CHECK("ncn_metrics_angles");
    hipLaunchKernelGGL(angles_reduce_kernel, dim3(1), dim3(MT_THREADS), 0, (hipStream_t)stream, ws, nb, sums, counts);
    NCN_LAUNCH_CHECK("ncn_metrics_angles (reduce)");
    return 0;
}

int ncn_select_median(const float* vals, int64_t capacity, int n_arrays, const int64_t* n_dev, uint32_t* ws,
                      int64_t ws_words, float* out, void* stream) {
    NCN_REQUIRE(vals != nullptr && n_dev != nullptr && out != nullptr && capacity >= 1 && capacity <= 0x7FFFFFFF &&
                    n_arrays >= 1 && n_arrays <= 65535,
                hipErrorInvalidValue, "ncn_select_median: bad arguments (capacity = %lld, n_arrays = %d)",
                (long long)capacity, n_arrays);
    NCN_REQUIRE(ws != nullptr && ws_words >= (int64_t)SEL_WORDS * n_arrays, hipErrorInvalidValue,
                "ncn_select_median: workspace of %lld words, %lld needed", (long long)ws_words,
                (long long)SEL_WORDS * n_arrays);
    hipStream_t s = (hipStream_t)stream;
    const int total = SEL_WORDS * n_arrays;
    hipLaunchKernelGGL(select_zero_kernel, dim3((unsigned)cdiv(total, SEL_THREADS)), dim3(SEL_THREADS), 0, s, ws, total);
    NCN_LAUNCH_CHECK("ncn_select_median (zero)");
    const unsigned nb = (unsigned)std::min<int64_t>(cdiv(capacity, SEL_THREADS * SEL_PER_THREAD), SEL_MAX_BLOCKS);
    for (int pass = 0; pass < 3; pass++) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(nb, (unsigned)n_arrays), dim3(SEL_THREADS), 0, s, vals, capacity, n_dev,
                           ws, pass);
        NCN_LAUNCH_CHECK("ncn_select_median (histogram)");
    }
    hipLaunchKernelGGL(select_pick_kernel, dim3((unsigned)n_arrays), dim3(SEL_THREADS), 0, s, capacity, n_dev, ws, out);
    NCN_LAUNCH_CHECK("ncn_select_median (pick)");
    return 0;
}

int ncn_metrics_finalise(const double* pw_sums, const int64_t* depth_count, int64_t n_rgb, const float* ssim,
                         const double* ang_sums, const int64_t* ang_counts, const float* medians, float* row,
                         void* stream) {
    NCN_REQUIRE(pw_sums != nullptr && ssim != nullptr && row != nullptr && n_rgb >= 1, hipErrorInvalidValue,
                "ncn_metrics_finalise: bad arguments");
    NCN_REQUIRE(ang_counts == nullptr || (ang_sums != nullptr && medians != nullptr), hipErrorInvalidValue,
                "ncn_metrics_finalise: ang_counts needs ang_sums and medians");
    hipLaunchKernelGGL(finalise_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, pw_sums, depth_count, n_rgb, ssim,
                       ang_sums, ang_counts, medians, row);
    NCN_LAUNCH_CHECK("ncn_metrics_finalise");
    return 0;
}

int ncn_sem_confusion(const float* logits, int64_t row_stride, const int64_t* labels, int label_shift,
                      int ignore_label, int64_t n_pix, int n_cls, int64_t* conf, int64_t* counts,
                      int32_t* pred_labels, void* stream) {
    static_assert(SEM_MAX_CLS == NCN_SEM_MAX_CLASSES, "ncnerf_sem.h and metrics_sem.h disagree");
    NCN_REQUIRE(n_cls >= 1 && n_cls <= SEM_MAX_CLS, hipErrorInvalidValue, "ncn_sem_confusion: n_cls = %d, 1..%d", n_cls,
                SEM_MAX_CLS);
    NCN_REQUIRE(n_pix >= 0 && n_pix <= ((int64_t)1 << 40) && row_stride >= n_cls, hipErrorInvalidValue,
                "ncn_sem_confusion: bad sizes (n_pix = %lld, row_stride = %lld, n_cls = %d)", (long long)n_pix,
                (long long)row_stride, n_cls);
    NCN_REQUIRE(conf != nullptr && counts != nullptr, hipErrorInvalidValue, "ncn_sem_confusion: null output");
    if (n_pix == 0) return 0;
    NCN_REQUIRE(logits != nullptr && labels != nullptr, hipErrorInvalidValue, "ncn_sem_confusion: null input");
    hipLaunchKernelGGL(sem_confusion_kernel, dim3(stream_blocks(n_pix)), dim3(SEM_THREADS),
                       4 * (size_t)sem_lds_words(n_cls), (hipStream_t)stream, logits, row_stride, labels,
                       (int64_t)label_shift, (int64_t)ignore_label, n_pix, n_cls, conf, counts, pred_labels);
    NCN_LAUNCH_CHECK("ncn_sem_confusion");
    return 0;
}

int ncn_sem_finalise(const int64_t* conf, int n_cls, float* out, void* stream) {
    NCN_REQUIRE(n_cls >= 1 && n_cls <= SEM_MAX_CLS, hipErrorInvalidValue, "ncn_sem_finalise: n_cls = %d, 1..%d", n_cls,
                SEM_MAX_CLS);
    NCN_REQUIRE(conf != nullptr && out != nullptr, hipErrorInvalidValue, "ncn_sem_finalise: null argument");
    hipLaunchKernelGGL(sem_finalise_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, conf, n_cls, out);
    NCN_LAUNCH_CHECK("ncn_sem_finalise");
    return 0;
}

}  // extern "C"
