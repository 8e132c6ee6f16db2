// The SSIM pass of metrics.hip: one launch gives the partial sums (and, if asked, the per-pixel maps)
// of the two Gaussian SSIMs (11x11, sigma 1.5; data range 1 and data range R) and of the uniform 7x7
// SSIM with sample covariance (data range R).
//
// A workgroup owns a tile of 8 rows x 64 pixels x 3 channels.  It stages the tile of both images with
// a 5-pixel halo in LDS ((8 + 10) rows x (64 + 10) pixels x 3 floats x 2 images = 31 968 B, so five
// workgroups fit a CU's 160 KiB), straight from the (H*W, 3) pixel-major layout: a tile row is 222
// consecutive floats in memory and in LDS.  Thread t owns column element t = 3 * x + c and all 8
// output rows of it.  For every staged row it takes the 11-tap horizontal sums of the five maps
// (p, t, p^2, t^2, p t) — lanes read consecutive LDS words (stride 3 floats between taps), so no bank
// is hit twice — and adds them, weighted, into the output rows they belong to: the vertical pass
// runs in registers and no filtered map is ever stored.  The 7x7 window takes taps 2..8 of the same
// loads and products.
//
// Cancellation: sigma = E[x^2] - mu^2 in f32 loses everything on a flat bright region.  Variances
// and covariances are shift invariant, so each thread subtracts the value of ITS column element at
// the tile's middle row from everything it reads; mu gets the shift back.
#pragma once
#include "workgroup.h"

namespace ncn {

constexpr int SS_TW = 64, SS_TH = 8;    // output tile, pixels
constexpr int SS_R = 5, SS_TAPS = 11;   // Gaussian window
constexpr int SS_RB = 3;                // 7x7 window
constexpr int SS_ROWS = SS_TH + 2 * SS_R;
constexpr int SS_LD = (SS_TW + 2 * SS_R) * 3;
constexpr int SS_THREADS = SS_TW * 3;

struct SsimTaps {
    float g[SS_R + 1];  // g[|d|], d = -5..5
    float eps;          // sum over the 11 x 11 window of fl32(g_i g_j), minus 1
};

// S of the definition from the window means of the SHIFTED values (e0 = E[p'], e1 = E[t'],
// e2 = E[p'^2], e3 = E[t'^2], e4 = E[p' t']), the shifts sp, st and the covariance normalisation.
// eps = (sum of the window's weights) - 1: the f32 Gaussian taps do not sum to exactly 1, and the
// definition's E[x^2] - mu^2 is shift invariant only up to terms in eps, restored here in closed form
// (E[p' + sp] = e0 + sp (1 + eps), and so on), so that S is the definition's value and not that of a
// renormalised window.
__device__ __forceinline__ float ssim_value(float e0, float e1, float e2, float e3, float e4, float sp, float st,
                                            float eps, float cov_norm, float c1, float c2) {
    const float sp1 = sp * (1.0f + eps), st1 = st * (1.0f + eps);
    const float mp = sp1 + e0, mt = st1 + e1;
    const float vp = cov_norm * ((e2 - e0 * e0) - eps * (sp * (2.0f * e0 + sp1)));
    const float vt = cov_norm * ((e3 - e1 * e1) - eps * (st * (2.0f * e1 + st1)));
    const float vpt = cov_norm * ((e4 - e0 * e1) - eps * (sp * e1 + st * e0 + sp * st1));
    return ((2.0f * mp * mt + c1) * (2.0f * vpt + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2));
}

__global__ __launch_bounds__(SS_THREADS) void ssim_tile_kernel(const float* __restrict__ pred,
                                                               const float* __restrict__ gt, int H, int W,
                                                               const float* __restrict__ range, SsimTaps taps,
                                                               double* __restrict__ partials,
                                                               float* __restrict__ maps) {
    __shared__ float lp[SS_ROWS][SS_LD];
    __shared__ float lt[SS_ROWS][SS_LD];
    __shared__ double red[SS_THREADS / WAVE][3];
    __shared__ float gw[SS_TAPS];  // the taps by a run-time index
    const int t = threadIdx.x;
    if (t < SS_TAPS) gw[t] = taps.g[t < SS_R ? SS_R - t : t - SS_R];
    const int x0 = blockIdx.x * SS_TW, y0 = blockIdx.y * SS_TH;
    const int64_t row_len = 3 * (int64_t)W;
    const int64_t col0 = 3 * (int64_t)(x0 - SS_R);
    for (int idx = t; idx < SS_ROWS * SS_LD; idx += SS_THREADS) {
        const int r = idx / SS_LD, q = idx - r * SS_LD;
        const int gy = y0 - SS_R + r;
        const int64_t gc = col0 + q;
        float a = 0.0f, b = 0.0f;  // outside the image: never part of a window that counts
        if (gy >= 0 && gy < H && gc >= 0 && gc < row_len) {
            const int64_t o = gy * row_len + gc;
            a = pred[o];
            b = gt[o];
        }
        lp[r][q] = a;
        lt[r][q] = b;
    }
    __syncthreads();

    const int mid = min(y0 + SS_TH / 2, H - 1) - y0 + SS_R;
    const float sp = lp[mid][t + 3 * SS_R], st = lt[mid][t + 3 * SS_R];
    float ag[SS_TH][5], ab[SS_TH][5];
#pragma unroll
    for (int j = 0; j < SS_TH; j++) {
#pragma unroll
        for (int m = 0; m < 5; m++) ag[j][m] = ab[j][m] = 0.0f;
    }
    // (rolled over the staged rows: unrolled, the scheduler hoists the 396 LDS loads and spills; the
    // conditions on d are the same in every lane, so they are scalar branches)
#pragma unroll 1
    for (int r = 0; r < SS_ROWS; r++) {
        float hg[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, hb[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        const float* rp = &lp[r][t];
        const float* rt = &lt[r][t];
#pragma unroll
        for (int k = 0; k < SS_TAPS; k++) {
            const float p = rp[3 * k] - sp, q = rt[3 * k] - st;
            const float v[5] = {p, q, p * p, q * q, p * q};
            const float w = taps.g[k < SS_R ? SS_R - k : k - SS_R];
#pragma unroll
            for (int m = 0; m < 5; m++) {
                hg[m] = fmaf(w, v[m], hg[m]);
                if (k >= SS_R - SS_RB && k <= SS_R + SS_RB) hb[m] += v[m];
            }
        }
#pragma unroll
        for (int j = 0; j < SS_TH; j++) {
            const int d = r - j;  // the tap of output row j that staged row r is
            if (d >= 0 && d < SS_TAPS) {
                const float w = gw[d];
#pragma unroll
                for (int m = 0; m < 5; m++) ag[j][m] = fmaf(w, hg[m], ag[j][m]);
            }
            if (d >= SS_R - SS_RB && d <= SS_R + SS_RB) {
#pragma unroll
                for (int m = 0; m < 5; m++) ab[j][m] += hb[m];
            }
        }
    }

    const float R = range[1] - range[0];
    const float c1 = (0.01f * 1.0f) * (0.01f * 1.0f), c2 = (0.03f * 1.0f) * (0.03f * 1.0f);
    const float c1n = (0.01f * R) * (0.01f * R), c2n = (0.03f * R) * (0.03f * R);
    const float inv49 = 1.0f / 49.0f, norm7 = 49.0f / 48.0f;
    const int x = x0 + t / 3, c = t - 3 * (t / 3);
    const bool xg = x >= SS_R && x <= W - 1 - SS_R, xb = x >= SS_RB && x <= W - 1 - SS_RB;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < SS_TH; j++) {
        const int y = y0 + j;
        const int64_t o = ((int64_t)y * W + x) * 3 + c, plane = (int64_t)H * W * 3;
        if (xg && y >= SS_R && y <= H - 1 - SS_R) {
            const float a = ssim_value(ag[j][0], ag[j][1], ag[j][2], ag[j][3], ag[j][4], sp, st, taps.eps, 1.0f, c1, c2);
            const float b = ssim_value(ag[j][0], ag[j][1], ag[j][2], ag[j][3], ag[j][4], sp, st, taps.eps, 1.0f, c1n, c2n);
            s0 += a;
            s1 += b;
            if (maps != nullptr) {
                maps[o] = a;
                maps[plane + o] = b;
            }
        }
        if (xb && y >= SS_RB && y <= H - 1 - SS_RB) {
            const float e = ssim_value(ab[j][0] * inv49, ab[j][1] * inv49, ab[j][2] * inv49, ab[j][3] * inv49,
                                       ab[j][4] * inv49, sp, st, 0.0f, norm7, c1n, c2n);
            s2 += e;
            if (maps != nullptr) maps[2 * plane + o] = e;
        }
    }
    double s[3] = {(double)s0, (double)s1, (double)s2};
    block_sum<3, SS_THREADS>(s, red);
    if (t == 0) {
        double* out = partials + 3 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
        out[0] = s[0]; out[1] = s[1]; out[2] = s[2];
    }
}

}  // namespace ncn
