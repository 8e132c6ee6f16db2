// The clustering kernel: faiss.Kmeans(3, K, niter, spherical=True) + index.search (losses.py:86-89,
// arithmetic in kmeans_faiss.h, random draws precomputed in the host-built plan) + the Manhattan
// cluster selection + the cluster losses and their analytic gradient, in ONE persistent launch.
#pragma once
#include "cluster_lloyd.h"
#include "cluster_select.h"
#include "workgroup.h"

namespace ncn {

__device__ __forceinline__ bool valid_normal(float a, float b, float c) {
    const bool zero = (fabsf(a) + fabsf(b) + fabsf(c)) == 0.0f;
    const bool bad = isnan(a) || isnan(b) || isnan(c) || isinf(a) || isinf(b) || isinf(c);
    return !(zero || bad);
}

template <int K>
struct ClusterLds {
    float pv[3][KM_CHUNK_MAX];  // this workgroup's chunk of the compacted normals (flip-signed after select)
    int pidx[KM_CHUNK_MAX];     // their original index
    int pk[KM_CHUNK_MAX];       // k-means assignment, then selected cluster 0..2 (-1 unselected)
    int plab[KM_CHUNK_MAX];     // selected label +-1..3 / 0
    unsigned long long acc[NCN_MAX_NQ];  // this workgroup's fixed-point sums of the phase
    unsigned long long accr[KM_ACC_COPIES][NCN_MAX_NQ];  // the Lloyd rounds' sums (per-lane copies)
    float C[K][3];
    float cnt[K];
    int label_map[K];
    int wcnt[CL_MAX_TRI / KM_THREADS][KM_THREADS / 64];
    int woff[CL_MAX_TRI / KM_THREADS][KM_THREADS / 64];
    int pick[K];       // init picks (ranks), sorted ascending
    int pick_ord[K];   // the centroid index of sorted pick k
    int picki[K];
    float pickv[K][3];  // the init picks' normals (register-resident compaction)
    unsigned char pmem[KM_CHUNK_MAX];  // training-set membership of the chunk's points (faiss subsampling)
    int total;
    int timed_out;  // the sticky status word, read once after the last grid barrier
    int late_drop;  // km_grid_exit's word
    KmUpdLds<K> upd;
    SelLds<K> sel;
    ClStats S;
    float st3[15];
    float G[3][3][3];  // G[term][cluster][xyz]
};

#ifdef NCN_DIAG_CL_TIMES
__device__ unsigned long long ncn_cl_times[64];
#define CL_STAMP(i) \
    if (bid == 0 && threadIdx.x == 0 && (i) < 64) ncn_cl_times[(i)] = __builtin_amdgcn_s_memrealtime()
#else
#define CL_STAMP(i)
#endif

// The buffers the Lloyd rounds of this launch do not write get void words (every launch writes
// every word of both buffers): both when nothing is clustered, the odd one when no round follows
// round 0.
template <int K>
__device__ __forceinline__ void cl_void_tags(const KmWs& ws, int bid, unsigned seq, bool clustered) {
    const long long vw = km_tagged(km_round_tag(seq, KM_VOID_ROUND), 0);
    for (int q = threadIdx.x; q < K * 4; q += KM_THREADS) {
        if (!clustered) st_c(ws.part + bid * K * 4 + q, vw);         // buffer 0
        st_c(ws.part + (KM_BLOCKS + bid) * K * 4 + q, vw);  // buffer 1
    }
}

// ---- select: final cluster sizes = count column of the final-search partials; cluster selection;
// label, flip sign and selected cluster per point; flipped member sums to p2 ----
template <int K>
__device__ __forceinline__ void cl_select_flip(ClusterLds<K>& L, const KmWs& ws, int bid, unsigned seq, int len,
                                               int niter_eff, float t_sim) {
    const int tid = threadIdx.x;
    if (tid < K)
        L.cnt[tid] = sum_rows_tagged(ws.part + (niter_eff & 1) * KM_BLOCKS * K * 4, K * 4, 4 * tid + 3,
                                     km_round_tag(seq, niter_eff), ws.sync);
    __syncthreads();
    CL_STAMP(57);
    select_clusters<K>(L.C, L.cnt, t_sim, L.sel, L.label_map);
    CL_STAMP(58);
    for (int j = tid; j < len; j += KM_THREADS) {
        const int lb = L.label_map[L.pk[j]];
        L.plab[j] = lb;
        const float sg = lb < 0 ? -1.f : 1.f;
        L.pk[j] = (lb < 0 ? -lb : lb) - 1;
        L.pv[0][j] *= sg;
        L.pv[1][j] *= sg;
        L.pv[2][j] *= sg;
    }
    if (tid < 12) L.acc[tid] = 0ull;
    __syncthreads();
    for (int j = tid; j < len; j += KM_THREADS) {
        const int c = L.pk[j];
        if (c < 0) continue;
#pragma unroll
        for (int q = 0; q < 3; q++) atomicAdd(&L.acc[4 * c + q], km_fix(L.pv[q][j]));
        atomicAdd(&L.acc[4 * c + 3], (unsigned long long)KM_FX);
    }
    __syncthreads();
    if (tid < 12) st_c(ws.p2 + bid * KM_P2_ROW + tid, (long long)L.acc[tid]);
}

// ---- sums: the selected clusters' statistics from p2, then per-cluster partials of x.c, |x-c|_1,
// sign(x-c) to p3 ----
template <int K>
__device__ __forceinline__ void cl_sums(ClusterLds<K>& L, const KmWs& ws, int bid, int len) {
    const int tid = threadIdx.x;
    CL_STAMP(59);
    cluster_stats(ws, L.S);
    CL_STAMP(61);
    if (L.S.ok) {
        if (tid < 15) L.acc[tid] = 0ull;
        __syncthreads();
        for (int j = tid; j < len; j += KM_THREADS) {
            const int c = L.pk[j];
            if (c < 0) continue;
            const float x0 = L.pv[0][j], x1 = L.pv[1][j], x2 = L.pv[2][j];
            const float* cc = L.S.cc[c];
            atomicAdd(&L.acc[5 * c], km_fix(x0 * cc[0] + x1 * cc[1] + x2 * cc[2]));
            atomicAdd(&L.acc[5 * c + 1], km_fix(fabsf(x0 - cc[0]) + fabsf(x1 - cc[1]) + fabsf(x2 - cc[2])));
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const float u = L.pv[q][j] - cc[q];
                atomicAdd(&L.acc[5 * c + 2 + q], km_fix(u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f)));
            }
        }
        __syncthreads();
        if (tid < 15) st_c(ws.p3 + bid * KM_P3_ROW + tid, (long long)L.acc[tid]);
    }
}

// ---- grad: the three cluster losses and their analytic gradient per point (losses.py:469-478),
// labels, the weight schedule of losses.py:217 and the loss total ----
template <int K>
__device__ __forceinline__ void cl_grad(ClusterLds<K>& L, const KmWs& ws, int bid, bool clustered, int nv, int len, int64_t T3,
                                        float w_ort, float w_dot, float w_l1, const float* __restrict__ w_dev,
                                        const int64_t* __restrict__ step_dev, float sched_start, float sched_grow,
                                        const float* __restrict__ photo, float* __restrict__ out_losses,
                                        int32_t* __restrict__ out_labels, float* __restrict__ out_centroids,
                                        float* __restrict__ dn) {
    const int tid = threadIdx.x;
    if (w_dev) { w_ort = w_dev[0]; w_dot = w_dev[1]; w_l1 = w_dev[2]; }
    if (step_dev) {  // losses.py:217: max(0, min(w, (step - start) * (w / grow)))
        const float ds = (float)(*step_dev) - sched_start;
        w_ort = fmaxf(0.f, fminf(w_ort, ds * (w_ort / sched_grow)));
        w_dot = fmaxf(0.f, fminf(w_dot, ds * (w_dot / sched_grow)));
        w_l1 = fmaxf(0.f, fminf(w_l1, ds * (w_l1 / sched_grow)));
    }
    // A barrier / hand-off timeout (this launch's or an earlier one's: the word is sticky until the
    // host clears it) means the partial sums may be incomplete.  The cluster terms are then dropped
    // as the reference's validity filter drops an invalid term (losses.py:246-262): losses 0, no
    // gradient, so no corrupt gradient is ever applied while the host's periodic status read
    // (losses.check_cluster_status) is pending.  Read after the last grid barrier: every flag store
    // is drained (vmcnt(0)) by the storing wave before its workgroup's next arrival, so a workgroup
    // whose data depends on a timed-out one sees the word.
    if (tid == 0)
        L.timed_out = (int)__hip_atomic_load(&ws.sync[KM_SYNC_STATUS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const bool ok = clustered && L.S.ok && L.timed_out == 0;
    if (bid == 0 && tid < K * 3) out_centroids[tid] = clustered ? (&L.C[0][0])[tid] : 0.f;
    if (tid == 0) {
        float ort = 0.f, cdot = 0.f, cl1 = 0.f;
        if (ok) {
            const float(*cc)[3] = L.S.cc;
            const float d12 = cc[0][0] * cc[1][0] + cc[0][1] * cc[1][1] + cc[0][2] * cc[1][2];
            const float d13 = cc[0][0] * cc[2][0] + cc[0][1] * cc[2][1] + cc[0][2] * cc[2][2];
            const float d23 = cc[1][0] * cc[2][0] + cc[1][1] * cc[2][1] + cc[1][2] * cc[2][2];
            ort = (fabsf(d12) + fabsf(d13) + fabsf(d23)) / 3.0f;
            for (int c = 0; c < 3; c++) {
                cdot += 1.0f - L.st3[5 * c] / L.S.cnt[c];
                cl1 += L.st3[5 * c + 1] / L.S.cnt[c];
            }
            cdot /= 3.0f;
            cl1 /= 3.0f;
            // upstream gradient w.r.t. each centroid c_k, per term
            const float s12 = d12 > 0.f ? 1.f : (d12 < 0.f ? -1.f : 0.f);
            const float s13 = d13 > 0.f ? 1.f : (d13 < 0.f ? -1.f : 0.f);
            const float s23 = d23 > 0.f ? 1.f : (d23 < 0.f ? -1.f : 0.f);
            for (int q = 0; q < 3; q++) {
                const float go[3] = {(s12 * cc[1][q] + s13 * cc[2][q]) / 3.0f,
                                     (s12 * cc[0][q] + s23 * cc[2][q]) / 3.0f,
                                     (s13 * cc[0][q] + s23 * cc[1][q]) / 3.0f};
                for (int c = 0; c < 3; c++) {
                    L.G[0][c][q] = w_ort * go[c];
                    L.G[1][c][q] = (w_dot / 3.0f) * (-L.S.cm[c][q]);
                    L.G[2][c][q] = (w_l1 / 3.0f) * (-L.st3[5 * c + 2 + q] / L.S.cnt[c]);
                }
            }
            // project through c = m/|m| : dL/dm = (G - c (c.G)) / |m|, then dm/dx = 1/N
            for (int tm = 0; tm < 3; tm++)
                for (int c = 0; c < 3; c++) {
                    const float cg = cc[c][0] * L.G[tm][c][0] + cc[c][1] * L.G[tm][c][1] + cc[c][2] * L.G[tm][c][2];
                    for (int q = 0; q < 3; q++)
                        L.G[tm][c][q] = (L.G[tm][c][q] - cc[c][q] * cg) / (fmaxf(L.S.cmn[c], 1e-12f) * L.S.cnt[c]);
                }
        }
        if (bid == 0) {
            out_losses[0] = ort; out_losses[1] = cdot; out_losses[2] = cl1; out_losses[3] = (float)nv;
            out_losses[4] = w_ort * ort; out_losses[5] = w_dot * cdot; out_losses[6] = w_l1 * cl1;
            out_losses[7] = w_ort; out_losses[8] = w_dot; out_losses[9] = w_l1;
            if (photo) {  // `total` in the order of losses.py's sum over the loss dict
                float tot = 0.f;
                tot += photo[0];
                tot += photo[1];
                tot += out_losses[4];
                tot += out_losses[5];
                tot += out_losses[6];
                out_losses[10] = tot;
            }
        }
    }
    __syncthreads();
    // per-normal label and gradient (direct terms + through the centroid), times the flip sign
    for (int j = tid; j < len; j += KM_THREADS) {
        const int i = L.pidx[j];
        const int lb = clustered ? L.plab[j] : 0;
        out_labels[i] = lb;
        const int c = clustered ? L.pk[j] : -1;
        if (!ok || c < 0) {
#pragma unroll
            for (int q = 0; q < 3; q++) dn[3 * i + q] = dn[T3 + 3 * i + q] = dn[2 * T3 + 3 * i + q] = 0.f;
            continue;
        }
        const float sg = lb < 0 ? -1.f : 1.f;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const float u = L.pv[q][j] - L.S.cc[c][q];
            const float su = u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f);
            dn[3 * i + q] = sg * L.G[0][c][q];
            dn[T3 + 3 * i + q] = sg * ((w_dot / 3.0f) * (-L.S.cc[c][q] / L.S.cnt[c]) + L.G[1][c][q]);
            dn[2 * T3 + 3 * i + q] = sg * ((w_l1 / 3.0f) * (su / L.S.cnt[c]) + L.G[2][c][q]);
        }
    }
    CL_STAMP(60);
}

// The whole clustering pipeline in ONE launch of KM_BLOCKS co-resident workgroups, the phases
// separated by the tagged hand-offs and grid barriers of cluster_ws.h instead of kernel boundaries:
//   compaction  (no barrier: every workgroup ranks all normals itself and keeps its chunk in LDS)
//               validity filter + ordered compaction (losses.py:427-430), faiss's training-set
//               membership and init picks from the plan
//   niter + 1 Lloyd rounds: C_i = update(partials_{i-1}, C_{i-1}) (i > 0), assign every point to
//               argmax <x, C_i>, per-workgroup partial sums (x, y, z, count) per cluster; the last
//               round (i = niter) is faiss's final search and keeps the assignment
//   select      cluster selection (losses.py:75-166) -> label per point, flipped partial sums
//   sums        per-cluster partials of x.c, |x-c|_1, sign(x-c)
//   grad        the three cluster losses and their analytic gradient per point (losses.py:469-478),
//               labels (-9 invalid), the weight schedule of losses.py:217 and the loss total
// Every workgroup reduces the same partials in the same fixed order, so all of them hold
// bit-identical centroids/statistics and the result is run-to-run deterministic.
// The body is a device function of the workgroup's index bid in [0, KM_BLOCKS) and its LDS, so that
// it can also run as one role of a wider launch (split_fused.hip); cluster_kernel below is the
// launch of its own.  All of the workgroup's LDS is L: nothing here declares __shared__ storage.
template <int K>
__device__ __forceinline__ void cluster_body(
    ClusterLds<K>& L, const int bid, const float* __restrict__ normals, int n_tri, int niter,
    const uint32_t* __restrict__ plan_words, float t_sim, float w_ort, float w_dot, float w_l1,
    const float* __restrict__ w_dev, const int64_t* __restrict__ step_dev, float sched_start, float sched_grow,
    const float* __restrict__ photo, float* __restrict__ wsb, float* __restrict__ out_losses,
    int32_t* __restrict__ out_labels, float* __restrict__ out_centroids, float* __restrict__ dn) {
    const KmWs ws = km_ws(wsb, K);
    constexpr int NW = KM_THREADS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t T3 = (int64_t)n_tri * 3;
    CL_STAMP(0);
    // ---- compaction: ranks of the valid normals in index order, this workgroup's chunk to LDS (its
    // loaded normals, flags and picks live in registers across the phase, so it stays in the kernel) ----
    const int R = (n_tri + KM_THREADS - 1) / KM_THREADS;  // <= 64 rounds
    // R <= 16 (n_tri <= 16 * KM_THREADS: 8192 at 512 threads; config #2 has 6272): the loaded
    // normals stay in registers and the chunk / init picks are stored from them (no second gather)
    const bool regs = R <= 16;
    uint64_t flags = 0;
    float a[16][3];
    for (int r0 = 0; r0 < R; r0 += 16) {  // 16 rounds of loads in flight before their ballots
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int i = (r0 + u) * KM_THREADS + tid;
            const bool in = r0 + u < R && i < n_tri;
#pragma unroll
            for (int q = 0; q < 3; q++) a[u][q] = in ? normals[3 * i + q] : 0.f;  // zero = invalid
        }
#pragma unroll
        for (int u = 0; u < 16; u++) {
            if (r0 + u >= R) break;  // uniform
            const bool v = valid_normal(a[u][0], a[u][1], a[u][2]);
            flags |= (uint64_t)v << (r0 + u);
            const uint64_t b = __ballot(v);
            if (lane == 0) L.wcnt[r0 + u][wid] = __popcll(b);
        }
    }
    __syncthreads();
    if (wid == 0) {  // exclusive scan of the R*NW counts in (round, wave) order: 4 per lane
        int v[4], sacc = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int q = 4 * lane + e;
            v[e] = q < R * NW ? (&L.wcnt[0][0])[q] : 0;
            sacc += v[e];
        }
        const int incl = wave_incl_sum(sacc, lane);
        int run = incl - sacc;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int q = 4 * lane + e;
            if (q < R * NW) (&L.woff[0][0])[q] = run;
            run += v[e];
        }
        if (lane == 63) L.total = incl;
    }
    __syncthreads();
    const int nv = L.total;
    const bool clustered = nv >= K;
    int m0, len;
    km_chunk(bid, nv, m0, len);
    KmPlan plan;
    plan.p = plan_words;
    const bool plan_ok = plan.n_tri() == n_tri && plan.K() == K;
    if (!plan_ok && tid == 0) km_set_status(ws.sync, 3u);
    // faiss: training set = rand_perm(seed) subsample of nv > K*256 points; nv == K is its copy corner
    // case (centroids = the points, no iteration)
    const int n_train = (plan_ok && nv > plan.cap()) ? plan.cap() : nv;
    const int niter_eff = n_train == K ? 0 : niter;
    // init picks (plan: first K of rand_perm(seed + 1)), loaded by K threads at once, then sorted
    // with their index by rank (thread k: its position = the picks below it, ties in index order —
    // the order of a stable sort; one LDS pass per thread instead of a serial insertion sort, whose
    // dependent LDS round trips cost ~5 us in one thread)
    if (clustered && tid < K) L.picki[tid] = plan_ok ? plan.init(nv, tid) : tid;
    __syncthreads();
    if (clustered && tid < K) {
        const int v = L.picki[tid];
        int rk = 0;
#pragma unroll
        for (int j = 0; j < K; j++) {
            const int u = L.picki[j];
            rk += (u < v || (u == v && j < tid)) ? 1 : 0;
        }
        L.pick[rk] = v;
        L.pick_ord[rk] = tid;
    }
    for (int j = tid; j < len; j += KM_THREADS) L.pmem[j] = plan_ok ? plan.member(nv, m0 + j) : 1;
    __syncthreads();
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int picks[K];
#pragma unroll
    for (int k = 0; k < K; k++) picks[k] = clustered ? __builtin_amdgcn_readfirstlane(L.pick[k]) : -1;
    CL_STAMP(56);
    // per-lane copies for the round loop: lane r holds round r's first rank, lane k pick k (sorted),
    // so a round's rank range is two readlanes and its picks two ballots (no LDS round trip and no
    // K-long scalar scan per round)
    const int wo_lane = lane < R ? L.woff[lane][0] : nv;
    const int pk_lane = (clustered && lane < K) ? L.pick[lane] : INT_MAX;
    auto rank_round = [&](int r, const float* ar) {
        // uniform skip of the rounds that hold neither a rank of this chunk, nor an init pick, nor
        // invalid normals this workgroup labels
        const int rlo = __builtin_amdgcn_readlane(wo_lane, r);
        const int rhi = r + 1 < R ? __builtin_amdgcn_readlane(wo_lane, r + 1) : nv;
        // the (sorted) picks inside [rlo, rhi): k in [kbeg, kend)
        const int kbeg = (int)__popcll(__ballot(pk_lane < rlo)), kend = (int)__popcll(__ballot(pk_lane < rhi));
        if (!(rlo < m0 + len && rhi > m0) && r % KM_BLOCKS != bid && kbeg == kend) return;
        const bool v = (flags >> r) & 1u;
        const int rank = L.woff[r][wid] + __popcll(__ballot(v) & lt);
        if (v) {
            const int i = r * KM_THREADS + tid;
            if (rank >= m0 && rank < m0 + len) {
                L.pidx[rank - m0] = i;
                if (ar) {
#pragma unroll
                    for (int q = 0; q < 3; q++) L.pv[q][rank - m0] = ar[q];
                }
            }
            for (int k = kbeg; k < kend; k++)  // usually none or one
                if (picks[k] == rank) {
                    L.picki[L.pick_ord[k]] = i;
                    if (ar) {
#pragma unroll
                        for (int q = 0; q < 3; q++) L.pickv[L.pick_ord[k]][q] = ar[q];
                    }
                }
        } else if (r * KM_THREADS + tid < n_tri && r % KM_BLOCKS == bid) {  // invalid: label -9, zero grad
            const int i = r * KM_THREADS + tid;
            out_labels[i] = -9;
#pragma unroll
            for (int q = 0; q < 3; q++) dn[3 * i + q] = dn[T3 + 3 * i + q] = dn[2 * T3 + 3 * i + q] = 0.f;
        }
    };
    if (regs) {
#pragma unroll
        for (int r = 0; r < 16; r++)
            if (r < R) rank_round(r, a[r]);  // (uniform; register indices are compile-time)
    } else {
        for (int r = 0; r < R; r++) rank_round(r, nullptr);
    }
    __syncthreads();
    if (!regs)
        for (int j = tid; j < len; j += KM_THREADS) {  // this chunk's normals and the init centroids
            const int i = L.pidx[j];
#pragma unroll
            for (int q = 0; q < 3; q++) L.pv[q][j] = normals[3 * i + q];
        }
    if (clustered && tid < K) {
        // faiss Clustering::train: centroids = the picked points, then post_process_centroids
        // (renormalised) BEFORE the iteration loop, so also at niter = 0; only the nx == k corner
        // returns the copied points untouched
        float c[3];
#pragma unroll
        for (int q = 0; q < 3; q++) c[q] = regs ? L.pickv[tid][q] : normals[3 * L.picki[tid] + q];
        if (n_train != K) faiss_renorm3(c);
#pragma unroll
        for (int q = 0; q < 3; q++) L.C[tid][q] = c[q];
    }
    __syncthreads();
    CL_STAMP(1);
    unsigned phase = 0;
    const unsigned seq = __hip_atomic_load(&ws.sync[KM_SYNC_SEQ], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!clustered || niter_eff == 0) cl_void_tags<K>(ws, bid, seq, clustered);
    if (clustered) {
        // ---- niter + 1 Lloyd rounds (hand-off: tagged words, no grid barrier; the loop stays in the kernel:
        // as a function it costs cluster_kernel<10> a register) ----
        for (int it = 0; it <= niter_eff; it++) {
            if (it > 0) {  // (clears L.accr behind its barrier)
                km_update<K>(ws.part + ((it - 1) & 1) * KM_BLOCKS * K * 4, L.C, L.upd, &L.accr[0][0],
                             km_round_tag(seq, it - 1), ws.sync, plan, n_train);
            } else {
                if (tid < K * 4) {
#pragma unroll
                    for (int c = 0; c < KM_ACC_COPIES; c++) L.accr[c][tid] = 0ull;
                }
                if (tid == 0) L.upd.emp[1] = 0;  // (K * 4 <= 64: wave 1 never writes it)
                __syncthreads();
            }
            CL_STAMP(2 + 2 * it);
            // assignment + per-cluster (x, y, z, count) sums of the chunk (fixed point, LDS u64 atomics):
            // training rounds over the training set, the final search (it == niter_eff) over all points
            for (int j = tid; j < len; j += KM_THREADS) {
                const float x = L.pv[0][j], y = L.pv[1][j], z = L.pv[2][j];
                const int a = faiss_nearest(L.C, K, x, y, z);
                L.pk[j] = a;
                if (it < niter_eff && !L.pmem[j]) continue;
                unsigned long long* ac = L.accr[lane % KM_ACC_COPIES];
                atomicAdd(&ac[4 * a], faiss_fix(x));
                atomicAdd(&ac[4 * a + 1], faiss_fix(y));
                atomicAdd(&ac[4 * a + 2], faiss_fix(z));
                atomicAdd(&ac[4 * a + 3], (unsigned long long)FAISS_FXL);
            }
            __syncthreads();
            if (tid < K * 4) {
                unsigned long long sum = 0ull;
#pragma unroll
                for (int c = 0; c < KM_ACC_COPIES; c++) sum += L.accr[c][tid];
                st_c(ws.part + (it & 1) * KM_BLOCKS * K * 4 + bid * K * 4 + tid,
                     km_tagged(km_round_tag(seq, it), (long long)sum));
            }
            CL_STAMP(3 + 2 * it);
        }
        cl_select_flip<K>(L, ws, bid, seq, len, niter_eff, t_sim);
        km_grid_sync(ws.sync, ++phase);
        cl_sums<K>(L, ws, bid, len);
        km_grid_sync(ws.sync, ++phase);  // uniform: S.ok is the same in every workgroup
        CL_STAMP(62);
        if (L.S.ok) sum_partials(ws.p3, KM_P3_ROW, 15, L.st3);
        __syncthreads();
        CL_STAMP(63);
    }
    cl_grad<K>(L, ws, bid, clustered, nv, len, T3, w_ort, w_dot, w_l1, w_dev, step_dev, sched_start, sched_grow, photo, out_losses,
               out_labels, out_centroids, dn);
    // every launch (clustered or not) advances the tag sequence; the last workgroup out re-reads the
    // status word and, when it is set, drops the cluster terms of the WHOLE launch (a workgroup that
    // read the word before a late timeout set it has applied its gradient rows: they are zeroed here)
    if (km_grid_exit(ws.sync, L.late_drop)) {
        for (int64_t i = tid; i < 3 * T3; i += KM_THREADS) dn[i] = 0.f;
        if (tid == 0) {
            out_losses[0] = out_losses[1] = out_losses[2] = 0.f;
            out_losses[4] = out_losses[5] = out_losses[6] = 0.f;
            if (photo) out_losses[10] = photo[0] + photo[1];
        }
    }
}

template <int K>
__global__ __launch_bounds__(KM_THREADS) void cluster_kernel(
    const float* __restrict__ normals, int n_tri, int niter, const uint32_t* __restrict__ plan_words, float t_sim,
    float w_ort, float w_dot,
    float w_l1, const float* __restrict__ w_dev, const int64_t* __restrict__ step_dev, float sched_start,
    float sched_grow, const float* __restrict__ photo, float* __restrict__ wsb, float* __restrict__ out_losses,
    int32_t* __restrict__ out_labels, float* __restrict__ out_centroids, float* __restrict__ dn) {
    __shared__ ClusterLds<K> L;
    cluster_body<K>(L, (int)blockIdx.x, normals, n_tri, niter, plan_words, t_sim, w_ort, w_dot, w_l1, w_dev, step_dev,
                    sched_start, sched_grow, photo, wsb, out_losses, out_labels, out_centroids, dn);
}

}  // namespace ncn
