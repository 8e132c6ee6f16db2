// Clustering stage: the Manhattan cluster selection from the final centroids, and the statistics of
// the three selected clusters.
#pragma once
#include "cluster_ws.h"

namespace ncn {

// Cluster selection of losses.py:75-166 from the final centroids and sizes -> label_map[K]
// (+-1..3 for the three orthogonal main clusters and their opposites, 0 otherwise).
template <int K>
struct SelLds {
    float sim[K][K];
    float cmin[K];
    int cargmin[K];
};

template <int K>
__device__ void select_clusters(const float (*C)[3], const float* cnt, float t_sim, SelLds<K>& L, int* label_map) {
    const int tid = threadIdx.x;
    for (int q = tid; q < K * K; q += KM_THREADS) {
        const int i = q / K, j = q % K;
        L.sim[i][j] = C[i][0] * C[j][0] + C[i][1] * C[j][1] + C[i][2] * C[j][2];
    }
    __syncthreads();
    int c1 = 0;  // biggest cluster (topk(sorted)[0]; ties -> lowest index)
    for (int k = 1; k < K; k++)
        if (cnt[k] > cnt[c1]) c1 = k;
    if (tid < K) {  // criteria[i][j] = |s(i,c1)| + |s(c1,j)| + |s(i,j)| ; min over i (first) per column j
        const int j = tid;
        float mn = 0.f;
        int mi = -1;
        for (int i = 0; i < K; i++) {
            const float cr = fabsf(L.sim[i][c1]) + fabsf(L.sim[c1][j]) + fabsf(L.sim[i][j]);
            if (mi < 0 || cr < mn) { mn = cr; mi = i; }
        }
        L.cmin[j] = mn;
        L.cargmin[j] = mi;
    }
    __syncthreads();
    if (tid < 64) {  // one wave: c2 = first argmin of cmin, its c3, then per-cluster labels
        // (wave-uniform serial scans over the K LDS values: independent broadcast loads and a short
        // compare chain, instead of 6 dependent cross-lane shuffles per argmin)
        auto first_argmin = [&](const float* v) {  // ties -> lowest index
            float b = v[0];
            int bi = 0;
#pragma unroll
            for (int k = 1; k < K; k++)
                if (v[k] < b) { b = v[k]; bi = k; }
            return bi;
        };
        const int c2 = first_argmin(L.cmin), c3 = L.cargmin[c2];
        const int cs[3] = {c1, c2, c3};
        // opposite of each main cluster: first argmin of sim[cs[q]][*]
        int co[3];
#pragma unroll
        for (int q = 0; q < 3; q++) co[q] = first_argmin(L.sim[cs[q]]);
        if (tid < K) {  // the sequential overwrite order of losses.py: main clusters, then opposites
            const int k = tid;
            int lab = 0;
            for (int q = 0; q < 3; q++)
                if (L.sim[cs[q]][k] > t_sim) lab = q + 1;
            for (int q = 0; q < 3; q++)
                if (-1.0f * L.sim[cs[q]][co[q]] > t_sim && L.sim[co[q]][k] > t_sim) lab = -(q + 1);
            label_map[k] = lab;
        }
    }
    __syncthreads();
}

// Per selected cluster: count, mean m, |m| and c = m/|m| from the p2 partials; ok = no empty cluster
// (the mean of an empty cluster is NaN -> every term filtered, losses.py:246-262).
struct ClStats {
    float st[12];
    float cnt[3], cm[3][3], cmn[3], cc[3][3];
    int ok;
};
__device__ void cluster_stats(const KmWs& ws, ClStats& S) {
    sum_partials(ws.p2, KM_P2_ROW, 12, S.st);
    __syncthreads();
    if (threadIdx.x == 0) {
        int ok = 1;
        for (int c = 0; c < 3; c++) {
            S.cnt[c] = S.st[4 * c + 3];
            if (S.cnt[c] == 0.f) ok = 0;
            for (int q = 0; q < 3; q++) S.cm[c][q] = S.cnt[c] > 0.f ? S.st[4 * c + q] / S.cnt[c] : 0.f;
            const float nr = sqrtf(S.cm[c][0] * S.cm[c][0] + S.cm[c][1] * S.cm[c][1] + S.cm[c][2] * S.cm[c][2]);
            S.cmn[c] = nr;
            for (int q = 0; q < 3; q++) S.cc[c][q] = S.cm[c][q] / fmaxf(nr, 1e-12f);
        }
        S.ok = ok;
    }
    __syncthreads();
}

}  // namespace ncn
