// Clustering stage: one faiss iteration's centroid update from the workgroups' tagged partials.
#pragma once
#include "cluster_ws.h"

namespace ncn {

// One faiss iteration's update (Clustering.cpp compute_centroids + split_clusters +
// post_process_centroids): centroid = sum * (1 / count); the empty clusters are split
// (faiss_split_clusters, the random floats from the plan); then every centroid is L2-renormalised.
// Lanes 4k..4k+3 of waves 0-1 sum (cluster k, component c) over the workgroups' tagged rows, the
// count and the components meet inside the quad (DPP), and the renormalised centroid goes to C
// with ONE workgroup barrier; the same float operations as compute-then-renorm (faiss_renorm3's
// order), so the result is bit-identical.  A rare empty cluster takes the serial split path
// (thread 0, from the means and counts in LDS) behind two more barriers; a split walk longer than
// the plan's table sets status 2.  The thread that published acc[t] last round clears it here (the
// next round's sums start from zero).
template <int CTRL>
__device__ __forceinline__ float km_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int Q>
__device__ __forceinline__ float km_quad_get(float v) { return km_dpp<Q | (Q << 2) | (Q << 4) | (Q << 6)>(v); }
template <int K>
struct KmUpdLds {
    float nc[K][3];
    float cnt[K];
    int emp[2];  // per wave: an empty cluster this round (waves 0 and 1)
};
template <int K>
__device__ void km_update(const long long* __restrict__ part, float (*C)[3], KmUpdLds<K>& L,
                          unsigned long long* __restrict__ acc, unsigned tag, unsigned* sync, const KmPlan& plan,
                          int n_train) {
    static_assert(K * 4 <= 128, "the sums of a round are taken by waves 0 and 1");
    const int t = threadIdx.x;
    if (t < K * 4) {  // (quads whole: K * 4 lanes)
#pragma unroll
        for (int c = 0; c < KM_ACC_COPIES; c++) acc[c * NCN_MAX_NQ + t] = 0ull;
        const int k = t >> 2, c = t & 3;
        const float v = sum_rows_tagged(part, K * 4, t, tag, sync);
        const float n = km_quad_get<3>(v);
        const float inv = n > 0.f ? 1.0f / n : 0.f;
        const float m = v * inv;  // (0 for an empty cluster)
        const float x0 = km_quad_get<0>(m), x1 = km_quad_get<1>(m), x2 = km_quad_get<2>(m);
        if (c < 3) L.nc[k][c] = m;
        else L.cnt[k] = n;
        const uint64_t em = __ballot(c == 3 && n == 0.f);
        if ((t & 63) == 0) L.emp[t >> 6] = em != 0;
        const float nr = faiss_norm2(x0, x1, x2);  // faiss_renorm3, this lane's component
        const float y = nr > 0.f ? m * faiss_inv_norm(nr) : m;
        if (c < 3) C[k][c] = y;
    }
    __syncthreads();
    if (L.emp[0] | L.emp[1]) {  // (uniform, rare)
        if (threadIdx.x == 0 && faiss_split_clusters(L.nc, L.cnt, K, n_train, plan.rnd(), plan.n_rand()))
            km_set_status(sync, 2u);
        __syncthreads();
        if (threadIdx.x < K) {
            const int k = threadIdx.x;
            float c[3] = {L.nc[k][0], L.nc[k][1], L.nc[k][2]};
            faiss_renorm3(c);
#pragma unroll
            for (int q = 0; q < 3; q++) C[k][q] = c[q];
        }
        __syncthreads();
    }
}

}  // namespace ncn
