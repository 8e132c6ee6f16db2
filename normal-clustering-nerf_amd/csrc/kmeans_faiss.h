// faiss.Kmeans(3, K, niter, spherical=True) as the reference calls it (losses.py:86-89), restated
// ONCE: the arithmetic, constants and random draws that must agree with faiss bit for bit (the
// algorithm of oracle/losses_ref.py:spherical_kmeans), for the training step's clustering kernel
// (loss.hip: cluster_*.h) and the evaluation's k-means (frame.hip) alike.
// faiss rounds every product and sum to f32; a fused multiply-add would change the last bit of a dot
// product and with it an argmax or a centroid, so contraction is off from here on in the including file.
#pragma once
#pragma clang fp contract(off)

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <random>
#include <unordered_map>
#include <vector>
#include <hip/hip_runtime.h>

namespace ncn {

constexpr int FAISS_MAX_PTS = 256;  // ClusteringParameters::max_points_per_centroid (subsampling cap = 256 K)
constexpr int FAISS_N_RAND = 4096;  // split_clusters' random floats handed to a kernel
// The Lloyd sums are exact: components of unit vectors are added as 64-bit fixed point v * 2^39
// (the count adds FAISS_FXL per point), so a sum does not depend on order or partition.
constexpr double FAISS_FXL = 549755813888.0;  // 2^39
__device__ __forceinline__ unsigned long long faiss_fix(float v) {
    return (unsigned long long)__double2ll_rn((double)v * FAISS_FXL);
}

// index.search: argmax_k <x, C_k> with ((x0 c0 + x1 c1) + x2 c2) in f32, no FMA; ties -> lowest k
// (a NaN point compares false everywhere and stays at 0).  faiss_nearest_step takes one candidate.
__device__ __forceinline__ float faiss_dot3(const float* c, float x, float y, float z) {
    return x * c[0] + y * c[1] + z * c[2];
}
__device__ __forceinline__ void faiss_nearest_step(const float* c, int k, float x, float y, float z, float& bv,
                                                   int& best) {
    const float v = faiss_dot3(c, x, y, z);
    if (v > bv) { bv = v; best = k; }
}
// (Tried in the clustering kernel: two clusters per packed-f32 instruction, v_pk_mul_f32 /
// v_pk_add_f32 with the same IEEE products and sums per half — 87 vs 82 us for the whole kernel:
// building the register pairs from the LDS centroids costs more than the halved multiplies save.)
__device__ __forceinline__ int faiss_nearest(const float (*C)[3], int K, float x, float y, float z) {
    int best = 0;
    float bv = faiss_dot3(C[0], x, y, z);
#pragma unroll
    for (int k = 1; k < K; k++) faiss_nearest_step(C[k], k, x, y, z, bv, best);
    return best;
}

// fvec_renorm_L2 of one 3-vector: x *= (float)(1.0 / sqrtf(|x|^2)) when |x|^2 > 0
__device__ __forceinline__ float faiss_norm2(float x0, float x1, float x2) { return x0 * x0 + x1 * x1 + x2 * x2; }
__device__ __forceinline__ float faiss_inv_norm(float nr) { return (float)(1.0 / (double)sqrtf(nr)); }
__device__ __forceinline__ void faiss_renorm3(float* x) {
    const float nr = faiss_norm2(x[0], x[1], x[2]);
    if (nr > 0.f) {
        const float inv = faiss_inv_norm(nr);
        x[0] *= inv; x[1] *= inv; x[2] *= inv;
    }
}

// Clustering.cpp split_clusters on one round's means nc[K][3] and (float) counts cnt[K], run by
// ONE thread: each empty cluster ci, in order, takes the cluster cj found by walking cj = 0, 1, ...
// (mod K) until rand_float() < (count_cj - 1) / (n_train - K) — the floats rnd[0..n_rand) of
// RandomGenerator(1234), from rnd[0] every round — a +-1/1024 perturbation splits the two, and the
// counts halve (as floats).  Returns whether a walk overran the floats (it takes the current cj and
// goes on; what to make of an overrun is the caller's policy).
__device__ __forceinline__ bool faiss_split_clusters(float (*nc)[3], float* cnt, int K, int n_train, const float* rnd,
                                                     int n_rand) {
    const float EPS = 1.0f / 1024.0f;
    const double denom = (double)(float)(n_train - K);
    int ri = 0;  // the next float; n_rand + 1 once a walk has overrun (every later walk then does too)
    for (int ci = 0; ci < K; ci++) {
        if (cnt[ci] != 0.f) continue;
        int cj = 0;
        for (;; cj = (cj + 1) % K) {
            const float pr = (float)(((double)cnt[cj] - 1.0) / denom);
            if (ri >= n_rand) { ri = n_rand + 1; break; }
            if (rnd[ri++] < pr) break;
        }
        for (int q = 0; q < 3; q++) {
            nc[ci][q] = nc[cj][q];
            if (q % 2 == 0) { nc[ci][q] *= 1 + EPS; nc[cj][q] *= 1 - EPS; }
            else { nc[ci][q] *= 1 - EPS; nc[cj][q] *= 1 + EPS; }
        }
        cnt[ci] = cnt[cj] / 2;
        cnt[cj] -= cnt[ci];
    }
    return ri > n_rand;
}

// ---- host: the random draws ----
// faiss rand_perm(perm, n, seed) (utils/random.cpp) for its first m steps, the first m entries to
// out: Fisher-Yates with RandomGenerator::rand_int(max) = mt() % max over std::mt19937((unsigned)seed).
// Up to FAISS_PERM_DENSE entries the permutation is held whole in `dense` (the caller's scratch: the
// k-means plan draws one prefix per point count); beyond, only the entries a swap touched are
// stored (<= 2 m), so n may be in the hundreds of millions.
constexpr int64_t FAISS_PERM_DENSE = 1 << 20;
template <class At, class Set>
inline void faiss_fisher_yates(int64_t n, uint32_t seed, int64_t m, At at, Set set) {
    std::mt19937 mt(seed);
    const int64_t steps = std::min(m, n - 1);
    for (int64_t i = 0; i < steps; i++) {
        const int64_t i2 = i + (int64_t)(mt() % (uint32_t)(n - i));
        const int64_t vi = at(i), v2 = at(i2);
        set(i, v2);
        set(i2, vi);
    }
}
inline void faiss_rand_perm_prefix(int64_t n, uint32_t seed, int64_t m, int64_t* out, std::vector<int32_t>& dense) {
    if (n <= FAISS_PERM_DENSE) {
        dense.resize((size_t)n);
        std::iota(dense.begin(), dense.end(), 0);
        faiss_fisher_yates(n, seed, m, [&](int64_t i) { return (int64_t)dense[i]; },
                           [&](int64_t i, int64_t v) { dense[i] = (int32_t)v; });
        for (int64_t i = 0; i < m; i++) out[i] = dense[i];
        return;
    }
    std::unordered_map<int64_t, int64_t> moved;
    moved.reserve((size_t)(2 * m));
    auto at = [&](int64_t i) {
        auto f = moved.find(i);
        return f == moved.end() ? i : f->second;
    };
    faiss_fisher_yates(n, seed, m, at, [&](int64_t i, int64_t v) { moved[i] = v; });
    for (int64_t i = 0; i < m; i++) out[i] = at(i);
}
// RandomGenerator(seed).rand_float() = mt() / float(mt.max()), n times
inline void faiss_rand_floats(uint32_t seed, int n, float* out) {
    std::mt19937 mt(seed);
    for (int i = 0; i < n; i++) out[i] = (float)mt() / (float)mt.max();
}

}  // namespace ncn
