// Manhattan-frame evaluation for gfx950 (the reference's validation path, train_nerf.py:381-534):
//  * per-pixel normals of a rendered depth image (datasets/hypersim_src/utils.py:544-611)
//  * faiss.Kmeans(3, K, niter, spherical=True) for any number of points: the random draws on the
//    host (ncn_kmeans_draws), the Lloyd rounds over the <= 256 K training points in ONE workgroup
//    (ncn_kmeans_train) and the final search of every point as a streaming pass (ncn_kmeans_assign).
// The algorithm is oracle/losses_ref.py:spherical_kmeans; its arithmetic, constants and draws are
// those of kmeans_faiss.h, shared with the training step's clustering kernel (loss.hip).  Nothing
// in this file waits on another workgroup.
#pragma clang fp contract(off)

#include <cstring>
#include "common.h"
#include "kmeans_faiss.h"
#include "../../include/ncnerf.h"

namespace ncn {

// ---- image normals ----
// One thread per pixel.  P = dirs_cc * depth (one f32 multiply per component), P1 the pixel, P2 the
// pixel above, P3 the pixel to the left; n = normalize(cross(P2 - P1, P3 - P1)) (F.normalize:
// / max(|.|, 1e-12)), rotated by the view's 3x3.  Border pixels and pixels whose own depth is 0,
// NaN or Inf are zero; a non-finite NEIGHBOUR leaves the NaN the arithmetic gives.
__global__ __launch_bounds__(256) void depth_normals_image_kernel(const float* __restrict__ depth,
                                                                  const float* __restrict__ dirs,
                                                                  const float* __restrict__ rot, int64_t total, int H,
                                                                  int W, float* __restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t hw = (int64_t)H * W;
    const int64_t b = i / hw, p = i - b * hw;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    const float d1 = depth[i];
    const bool inner = y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2;
    if (inner && !(d1 == 0.0f || isnan(d1) || isinf(d1))) {
        const float d2 = depth[i - W], d3 = depth[i - 1];
        const float* q1 = dirs + 3 * p;
        const float* q2 = dirs + 3 * (p - W);
        const float* q3 = dirs + 3 * (p - 1);
        const float P1x = q1[0] * d1, P1y = q1[1] * d1, P1z = q1[2] * d1;
        const float a0 = q2[0] * d2 - P1x, a1 = q2[1] * d2 - P1y, a2 = q2[2] * d2 - P1z;
        const float b0 = q3[0] * d3 - P1x, b1 = q3[1] * d3 - P1y, b2 = q3[2] * d3 - P1z;
        const float c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
        const float nrm = fmaxf(sqrtf(c0 * c0 + c1 * c1 + c2 * c2), 1e-12f);
        const float n0 = c0 / nrm, n1 = c1 / nrm, n2 = c2 / nrm;
        const float* R = rot + 9 * b;
        o0 = R[0] * n0 + R[1] * n1 + R[2] * n2;
        o1 = R[3] * n0 + R[4] * n1 + R[5] * n2;
        o2 = R[6] * n0 + R[7] * n1 + R[8] * n2;
    }
    normals[3 * i] = o0;
    normals[3 * i + 1] = o1;
    normals[3 * i + 2] = o2;
}

// ---- k-means ----
constexpr int KF_MAX_K = 32;
constexpr int KF_MAX_NITER = 64;
constexpr int KF_THREADS = 1024;    // the training workgroup
constexpr int KF_PER_THREAD = KF_MAX_K * FAISS_MAX_PTS / KF_THREADS;  // 8 points in registers
constexpr int KF_COPIES = 8;        // copies of the LDS accumulators (thread t adds into copy t % 8)

// faiss Clustering::train on the (already subsampled) training set, one workgroup: thread t holds
// points t, t + 1024, ... in registers; centroids, the exact int64 sums (x, y, z at 2^-39, count)
// and the round's means live in LDS.  Per round: search (faiss_nearest_step) + LDS integer atomics,
// mean = sum * (1 / count), faiss_split_clusters serially in thread 0, L2 renormalisation.
// nt == K is faiss's corner case: the points are the centroids.
// A split walk that runs past the FAISS_N_RAND floats has left the restated algorithm: the centroids
// are then written as NaN (never a value computed from different draws).
__global__ __launch_bounds__(KF_THREADS) void kmeans_train_kernel(const float* __restrict__ pts, int nt, int K,
                                                                  int niter, const int64_t* __restrict__ init_idx,
                                                                  const float* __restrict__ rnd,
                                                                  float* __restrict__ centroids) {
    __shared__ float C[KF_MAX_K][3];
    __shared__ float nc[KF_MAX_K][3];
    __shared__ float cnt[KF_MAX_K];
    __shared__ unsigned long long acc[KF_COPIES][KF_MAX_K][4];
    __shared__ int overrun;
    const int t = threadIdx.x;
    if (nt == K) {
        if (t < 3 * K) centroids[t] = pts[t];
        return;
    }
    float px[KF_PER_THREAD], py[KF_PER_THREAD], pz[KF_PER_THREAD];
#pragma unroll
    for (int j = 0; j < KF_PER_THREAD; j++) {
        const int i = t + j * KF_THREADS;
        const bool in = i < nt;
        px[j] = in ? pts[3 * i] : 0.f;
        py[j] = in ? pts[3 * i + 1] : 0.f;
        pz[j] = in ? pts[3 * i + 2] : 0.f;
    }
    if (t < K) {
        const int64_t s = init_idx[t];
        float c[3] = {pts[3 * s], pts[3 * s + 1], pts[3 * s + 2]};
        faiss_renorm3(c);
        C[t][0] = c[0]; C[t][1] = c[1]; C[t][2] = c[2];
    }
    if (t == 0) overrun = 0;
    unsigned long long* accf = &acc[0][0][0];
    for (int it = 0; it < niter; it++) {
        for (int q = t; q < KF_COPIES * KF_MAX_K * 4; q += KF_THREADS) accf[q] = 0ull;
        __syncthreads();
        unsigned long long(*my)[4] = acc[t & (KF_COPIES - 1)];
        // faiss_nearest for the thread's 8 points at once, clusters outermost: each centroid is read
        // from LDS once per thread and round (the same steps in the same cluster order per point)
        int best[KF_PER_THREAD];
        float bv[KF_PER_THREAD];
        {
            const float c[3] = {C[0][0], C[0][1], C[0][2]};
#pragma unroll
            for (int j = 0; j < KF_PER_THREAD; j++) {
                bv[j] = faiss_dot3(c, px[j], py[j], pz[j]);
                best[j] = 0;
            }
        }
        for (int k = 1; k < K; k++) {
            const float c[3] = {C[k][0], C[k][1], C[k][2]};
#pragma unroll
            for (int j = 0; j < KF_PER_THREAD; j++) faiss_nearest_step(c, k, px[j], py[j], pz[j], bv[j], best[j]);
        }
#pragma unroll
        for (int j = 0; j < KF_PER_THREAD; j++) {
            if (t + j * KF_THREADS < nt) {
                const int a = best[j];
                atomicAdd(&my[a][0], faiss_fix(px[j]));
                atomicAdd(&my[a][1], faiss_fix(py[j]));
                atomicAdd(&my[a][2], faiss_fix(pz[j]));
                atomicAdd(&my[a][3], 1ull);
            }
        }
        __syncthreads();
        if (t < K * 4) {
            const int k = t >> 2, c = t & 3;
            long long q = 0;
#pragma unroll
            for (int m = 0; m < KF_COPIES; m++) q += (long long)acc[m][k][c];
            long long qn = 0;
#pragma unroll
            for (int m = 0; m < KF_COPIES; m++) qn += (long long)acc[m][k][3];
            const float n = (float)qn;
            if (c == 3) {
                cnt[k] = n;
            } else {
                const float s = (float)((double)q * (1.0 / FAISS_FXL));
                nc[k][c] = n > 0.f ? s * (1.0f / n) : 0.f;
            }
        }
        __syncthreads();
        if (t == 0 && faiss_split_clusters(nc, cnt, K, nt, rnd, FAISS_N_RAND)) overrun = 1;
        __syncthreads();
        if (t < K) {
            float c[3] = {nc[t][0], nc[t][1], nc[t][2]};
            faiss_renorm3(c);
            C[t][0] = c[0]; C[t][1] = c[1]; C[t][2] = c[2];
        }
        __syncthreads();
    }
    __syncthreads();
    if (t < 3 * K) centroids[t] = overrun ? __int_as_float(0x7FC00000) : C[t / 3][t % 3];
}

// The final search (kmeans.index.search(x, 1)) of every point: a grid-stride stream, 12 B in and
// 4 B out per point, centroids in LDS, a per-workgroup LDS histogram flushed with one integer
// atomic per cluster (exact: independent of the grid and of the order).
// Every workgroup ends with K same-address global atomics, so the grid is kept small: at least 8
// points per thread, at most 1024 workgroups (4 per CU).
constexpr int KA_THREADS = 256;
constexpr int KA_PER_THREAD = 8;
constexpr int KA_MAX_BLOCKS = 1024;
__global__ void kmeans_zero_counts_kernel(unsigned long long* __restrict__ counts, int K) {
    if ((int)threadIdx.x < K) counts[threadIdx.x] = 0ull;
}
__global__ __launch_bounds__(KA_THREADS) void kmeans_assign_kernel(const float* __restrict__ pts, int64_t n,
                                                                   const float* __restrict__ centroids, int K,
                                                                   int32_t* __restrict__ assign,
                                                                   unsigned long long* __restrict__ counts) {
    __shared__ float C[KF_MAX_K][3];
    __shared__ unsigned long long hist[KF_MAX_K];
    const int t = threadIdx.x;
    if (t < 3 * K) C[t / 3][t % 3] = centroids[t];
    if (t < KF_MAX_K) hist[t] = 0ull;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * KA_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * KA_THREADS + t; i < n; i += stride) {
        const int a = faiss_nearest(C, K, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
        assign[i] = a;
        atomicAdd(&hist[a], 1ull);
    }
    __syncthreads();
    if (t < K && hist[t] != 0ull) atomicAdd(&counts[t], hist[t]);
}

}  // namespace ncn

using namespace ncn;

extern "C" {

int ncn_depth_normals_image(const float* depth, const float* dirs_cc, const float* rot, int B, int H, int W,
                            float* normals, void* stream) {
    NCN_REQUIRE(B >= 0 && H >= 1 && W >= 1, hipErrorInvalidValue, "ncn_depth_normals_image: bad shape %dx%dx%d", B, H, W);
    const int64_t total = (int64_t)B * H * W;
    if (total == 0) return 0;
    NCN_REQUIRE(cdiv(total, 256) <= 0x7FFFFFFF, hipErrorInvalidValue, "ncn_depth_normals_image: too many pixels");
    hipLaunchKernelGGL(depth_normals_image_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       depth, dirs_cc, rot, total, H, W, normals);
    NCN_LAUNCH_CHECK("ncn_depth_normals_image");
    return 0;
}

int ncn_kmeans_draws(int64_t nx, int K, uint32_t seed, int64_t* sub_idx, int64_t* init_idx, int64_t* init_rows) {
    NCN_REQUIRE(sub_idx != nullptr && init_idx != nullptr && K > 0 && K <= KF_MAX_K, hipErrorInvalidValue,
                "ncn_kmeans_draws: bad arguments (K = %d, at most %d)", K, KF_MAX_K);
    NCN_REQUIRE(nx >= K, hipErrorInvalidValue, "ncn_kmeans_draws: %lld points for %d clusters", (long long)nx, K);
    NCN_REQUIRE(nx <= 0x7FFFFFFF, hipErrorInvalidValue, "ncn_kmeans_draws: faiss's rand_perm takes an int count");
    const int64_t cap = (int64_t)K * FAISS_MAX_PTS, nt = std::min(nx, cap);
    std::vector<int32_t> scratch;
    if (nx > cap) {
        faiss_rand_perm_prefix(nx, seed, cap, sub_idx, scratch);  // subsample_training_set
    } else {
        for (int64_t i = 0; i < nt; i++) sub_idx[i] = i;
    }
    int64_t picks[KF_MAX_K];
    faiss_rand_perm_prefix(nt, seed + 1, K, picks, scratch);  // init, redo 0: seed + 1 + 0 * 15486557
    for (int k = 0; k < K; k++) {
        init_idx[k] = sub_idx[picks[k]];
        if (init_rows != nullptr) init_rows[k] = picks[k];
    }
    return 0;
}

int ncn_kmeans_rand_floats(uint32_t seed, int n, float* host_out) {
    NCN_REQUIRE(host_out != nullptr && n >= 0, hipErrorInvalidValue, "ncn_kmeans_rand_floats: bad arguments");
    faiss_rand_floats(seed, n, host_out);
    return 0;
}

int ncn_kmeans_train(const float* train_pts, int nt, int K, int niter, const int64_t* init_idx,
                     const float* rand_floats, float* centroids, void* stream) {
    NCN_REQUIRE(K > 0 && K <= KF_MAX_K, hipErrorInvalidValue, "ncn_kmeans_train: K = %d (1..%d)", K, KF_MAX_K);
    NCN_REQUIRE(nt >= K && nt <= K * FAISS_MAX_PTS, hipErrorInvalidValue,
                "ncn_kmeans_train: %d training points for K = %d (K..256 K; subsample with ncn_kmeans_draws)", nt, K);
    NCN_REQUIRE(niter >= 0 && niter <= KF_MAX_NITER, hipErrorInvalidValue, "ncn_kmeans_train: niter = %d (0..%d)", niter,
                KF_MAX_NITER);
    hipLaunchKernelGGL(kmeans_train_kernel, dim3(1), dim3(KF_THREADS), 0, (hipStream_t)stream, train_pts, nt, K, niter,
                       init_idx, rand_floats, centroids);
    NCN_LAUNCH_CHECK("ncn_kmeans_train");
    return 0;
}

int ncn_kmeans_assign(const float* pts, int64_t n, const float* centroids, int K, int32_t* assign, int64_t* counts,
                      void* stream) {
    NCN_REQUIRE(K > 0 && K <= KF_MAX_K && n >= 0, hipErrorInvalidValue, "ncn_kmeans_assign: bad arguments");
    hipLaunchKernelGGL(kmeans_zero_counts_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream,
                       (unsigned long long*)counts, K);
    NCN_LAUNCH_CHECK("ncn_kmeans_assign (zero counts)");
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(n, KA_THREADS * KA_PER_THREAD), KA_MAX_BLOCKS);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(blocks), dim3(KA_THREADS), 0, (hipStream_t)stream, pts, n, centroids,
                       K, assign, (unsigned long long*)counts);
    NCN_LAUNCH_CHECK("ncn_kmeans_assign");
    return 0;
}

}  // extern "C"
