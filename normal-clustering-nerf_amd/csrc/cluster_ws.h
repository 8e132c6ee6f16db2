// The clustering kernel's shared state, stated once (for the kernel's phases and loss.hip's ABI):
// launch shape, workspace, grid barrier, tagged Lloyd hand-off and the host-built k-means plan.
//   part  [2][KM_BLOCKS][K][4] tagged int64: each workgroup writes its row of buffer round & 1 every
//         Lloyd round; every workgroup reads all rows (km_update, the final cluster sizes)
//   p2    [KM_BLOCKS][12] int64 at 2^40: flipped member sums + counts per selected cluster; written
//         before grid barrier 1 (select), read after it (cluster_stats)
//   p3    [KM_BLOCKS][16] int64 at 2^40: x.c, |x-c|_1, sign(x-c) sums; written before barrier 2, read after
//   sync  [KM_SYNC_WORDS] u32: barrier arrivals, departures (both zero before the first call and after
//         every call), the sticky status word (ncn_cluster_status_offset), the tags' launch sequence
#pragma once
#include "common.h"
#include "kmeans_faiss.h"

namespace ncn {

constexpr int CL_MAX_TRI = 16384;
constexpr int NCN_MAX_NQ = 80;       // K * 4 at K = 20
#ifndef KM_THREADS_CFG
#define KM_THREADS_CFG 512
#endif
#ifndef KM_BLOCKS_CFG
#define KM_BLOCKS_CFG 16
#endif
constexpr int KM_THREADS = KM_THREADS_CFG;  // threads per workgroup of the clustering kernel
constexpr int KM_BLOCKS = KM_BLOCKS_CFG;    // co-resident workgroups (grid barriers)
constexpr int KM_CHUNK_MAX = CL_MAX_TRI / KM_BLOCKS;
// Copies of a Lloyd round's per-cluster LDS accumulators: lane l adds into copy l % KM_ACC_COPIES,
// so the lanes of one wave that picked the same cluster (same-address u64 atomics serialise) are
// spread over the copies; the publishing thread sums its word's copies (exact integers: the result
// does not depend on the split).
#ifndef KM_ACC_COPIES
#define KM_ACC_COPIES 4
#endif

// ---- workspace layout (32-bit words; the int64 parts first, so they stay 8-byte aligned) ----
enum { KM_SYNC_ARRIVE = 0, KM_SYNC_DEPART = 1, KM_SYNC_STATUS = 2, KM_SYNC_SEQ = 3, KM_SYNC_WORDS = 4 };
constexpr int KM_P2_ROW = 12, KM_P3_ROW = 16;
__host__ __device__ constexpr int64_t km_part_i64(int K) { return 2 * KM_BLOCKS * K * 4; }
__host__ __device__ constexpr int64_t km_sync_word(int K) {
    return 2 * (km_part_i64(K) + KM_BLOCKS * (KM_P2_ROW + KM_P3_ROW));
}
__host__ __device__ constexpr int64_t km_ws_words(int K) { return km_sync_word(K) + KM_SYNC_WORDS; }
__host__ __device__ constexpr int64_t km_status_word(int K) { return km_sync_word(K) + KM_SYNC_STATUS; }
struct KmWs {
    long long* part;
    long long* p2;
    long long* p3;
    unsigned* sync;
};
__host__ __device__ inline KmWs km_ws(float* base, int K) {
    KmWs w;
    w.part = (long long*)base;
    w.p2 = w.part + km_part_i64(K);
    w.p3 = w.p2 + KM_BLOCKS * KM_P2_ROW;
    w.sync = (unsigned*)(w.p3 + KM_BLOCKS * KM_P3_ROW);
    return w;
}

// Every sum of the barrier phases (select, sums) is exact: values (all |v| <= 8) are added as 64-bit
// fixed point v * 2^40 (LDS u64 atomics inside a workgroup, then int64 partials across workgroups),
// so the result is independent of order and partition, and is rounded to f32 once.
constexpr double KM_FX = 1099511627776.0;  // 2^40
__device__ __forceinline__ unsigned long long km_fix(float v) {
    return (unsigned long long)__double2ll_rn((double)v * KM_FX);
}
__device__ __forceinline__ float km_unfix(long long q) { return (float)((double)q * (1.0 / KM_FX)); }

// Cross-workgroup data moves with agent-scope (sc1) loads and stores only (MI355X_MICROARCH.md,
// inter-workgroup visibility, hand-off row 1): each storing wave waits for its stores, the
// workgroup meets at a barrier, ONE lane adds to the arrival counter; the poller's workgroup meets
// again before any sc1 load of the published bytes.
__device__ __forceinline__ long long ld_c(const long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_c(long long* p, long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The sticky status word: 1 a barrier / hand-off timed out, 2 a split walk ran past the plan's
// floats, 3 the plan does not belong to this (n_tri, K).
__device__ __forceinline__ void km_set_status(unsigned* sync, unsigned code) {
    __hip_atomic_store(&sync[KM_SYNC_STATUS], code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Grid barrier number `phase` (1, 2, ...) over the KM_BLOCKS co-resident workgroups.  The spin is
// bounded: a barrier that does not complete within ~2^22 polls sets the status word (sticky;
// ncn_cluster_status_offset) and lets the workgroup run on (never a hang); the launch then
// drops its cluster terms (zero losses and gradients, the grad phase), and the training step
// reads the word every few steps and raises (losses.check_cluster_status).
// NCN_KM_SPIN_LIMIT / NCN_KM_POLL_LIMIT: diagnostic builds force the flag with a limit of 1.
#ifndef NCN_KM_SPIN_LIMIT
#define NCN_KM_SPIN_LIMIT (1u << 22)
#endif
#ifndef NCN_KM_POLL_LIMIT
#define NCN_KM_POLL_LIMIT (1u << 20)
#endif
__device__ __forceinline__ void km_grid_sync(unsigned* sync, unsigned phase) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(&sync[KM_SYNC_ARRIVE], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned target = phase * (unsigned)KM_BLOCKS;
        unsigned spins = 0;
        while (__hip_atomic_load(&sync[KM_SYNC_ARRIVE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins >= NCN_KM_SPIN_LIMIT) { km_set_status(sync, 1u); break; }
        }
    }
    __syncthreads();
}
// Every workgroup calls this once, last: the final departure resets the barrier words and advances
// the launch sequence of the Lloyd tags (every launch, so a launch that did not cluster never
// leaves the next one with the tags of an older launch's partials).  Returns (to every thread of
// the LAST departing workgroup only) whether the status word is set: every workgroup's output
// stores are drained (vmcnt(0)) before its departure, so that workgroup can still overwrite the
// whole launch's outputs — the drop decision is then uniform even when a workgroup timed out after
// another one had read the word.  late_drop: one LDS word of the workgroup (ClusterLds).
__device__ __forceinline__ bool km_grid_exit(unsigned* sync, int& late_drop) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        late_drop = 0;
        const unsigned d = __hip_atomic_fetch_add(&sync[KM_SYNC_DEPART], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (d == KM_BLOCKS - 1) {  // everyone has passed every barrier: nobody polls any more
            late_drop = __hip_atomic_load(&sync[KM_SYNC_STATUS], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != 0u;
            __hip_atomic_store(&sync[KM_SYNC_ARRIVE], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&sync[KM_SYNC_DEPART], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&sync[KM_SYNC_SEQ], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    return late_drop != 0;
}

// Workgroup bid's contiguous chunk of the compacted points.
__device__ __forceinline__ void km_chunk(int bid, int nv, int& m0, int& len) {
    const int chunk = (nv + KM_BLOCKS - 1) / KM_BLOCKS;
    m0 = bid * chunk;
    len = max(0, min(nv, m0 + chunk) - m0);
}

// Exact sum of KM_BLOCKS int64 partial rows published by other workgroups (all loads issued
// before the first add: one round trip), as f32.
__device__ __forceinline__ float sum_rows(const long long* __restrict__ p, int row, int off) {
    long long v[KM_BLOCKS];
#pragma unroll
    for (int b = 0; b < KM_BLOCKS; b++) v[b] = ld_c(p + b * row + off);
    long long a = 0;
#pragma unroll
    for (int b = 0; b < KM_BLOCKS; b++) a += v[b];
    return km_unfix(a);
}
__device__ __forceinline__ void sum_partials(const long long* __restrict__ p, int row, int nq, float* out) {
    if (threadIdx.x < nq) out[threadIdx.x] = sum_rows(p, row, threadIdx.x);
}

// Lloyd-round partials are published as TAGGED words instead of behind a grid barrier: each
// int64 word = tag << 51 | (fixed-point value mod 2^51), value = sum * FAISS_FXL (2^39), read back
// as a SIGNED 51-bit field.  A workgroup sums at most KM_CHUNK_MAX = 1024 components of unit normals
// (|x| <= 1; the count word adds 1.0 per point), so |value| <= 1024 * 2^39 = 2^49, reached with
// either sign when a whole chunk is one cluster of axis-aligned normals (a wall in a patch-ordered
// batch); the field holds [-2^50, 2^50) (static_assert below).  (A 50-bit field, [-2^49, 2^49),
// read +2^49 as -2^49.)  The precision of the barrier-based 2^40 sums within a factor 2.
// tag (13 bits) = ((launch sequence + 1) mod 2^8) << 5 | round.  What a reader of (sequence s,
// round it) can find in a word of buffer it & 1: this launch's rounds it - 2, it - 4, ... or its
// void word (another round field: rounds are 0..30, void is 31); never this launch's round it + 2
// (double buffering, below); or the previous launch's word (sequence s - 1: another sequence field
// for any width >= 1 bit).  Nothing older: every launch writes every word of both buffers (a
// launch that does not cluster, or clusters with no Lloyd round, writes void tags), so a word is
// never older than the previous launch and the 8 sequence bits cannot alias when they wrap.
// So a reader polls the words themselves until all KM_BLOCKS rows carry the round's tag: one
// store and (usually) one load round trip per round instead of store + arrive + poll + load.
// The rows are double-buffered by round parity: a workgroup writes round it+2 only after it read
// round it+1 from every workgroup, each of which published it+1 only after reading round it.
constexpr int KM_TAG_SHIFT = 51;
constexpr int KM_ROUND_BITS = 5;
constexpr int KM_SEQ_BITS = 64 - KM_TAG_SHIFT - KM_ROUND_BITS;
constexpr unsigned long long KM_VMASK = (1ull << KM_TAG_SHIFT) - 1;
constexpr unsigned KM_VOID_ROUND = 31;  // round field of the void words (niter <= 30)
static_assert((double)KM_CHUNK_MAX * FAISS_FXL <= (double)((1ull << (KM_TAG_SHIFT - 1)) - 1),
              "a workgroup's Lloyd partial (KM_CHUNK_MAX unit components at scale FAISS_FXL) must fit the signed value field");
static_assert(KM_SEQ_BITS >= 1 && KM_VOID_ROUND < (1u << KM_ROUND_BITS), "tag = sequence | round");
__device__ __forceinline__ long long km_tagged(unsigned tag, long long v) {
    return (long long)(((unsigned long long)tag << KM_TAG_SHIFT) | ((unsigned long long)v & KM_VMASK));
}
__device__ __forceinline__ unsigned km_round_tag(unsigned seq, int it) {
    return (((seq + 1u) & ((1u << KM_SEQ_BITS) - 1u)) << KM_ROUND_BITS) | (unsigned)it;
}
// Exact sum of the KM_BLOCKS tagged words p[b * row + off] once every one carries `tag` (bounded
// poll: a row that never arrives sets the status word, as km_grid_sync does).
__device__ __forceinline__ float sum_rows_tagged(const long long* __restrict__ p, int row, int off, unsigned tag,
                                                 unsigned* sync) {
    long long v[KM_BLOCKS];
    for (unsigned spins = 0;; spins++) {
#pragma unroll
        for (int b = 0; b < KM_BLOCKS; b++) v[b] = ld_c(p + b * row + off);
        bool ready = true;
#pragma unroll
        for (int b = 0; b < KM_BLOCKS; b++) ready &= ((unsigned long long)v[b] >> KM_TAG_SHIFT) == tag;
        if (ready) break;
        if (spins + 1 >= NCN_KM_POLL_LIMIT) { km_set_status(sync, 1u); break; }
        __builtin_amdgcn_s_sleep(1);
    }
    long long a = 0;
#pragma unroll
    for (int b = 0; b < KM_BLOCKS; b++)  // sign-extend the KM_TAG_SHIFT-bit values
        a += (long long)((unsigned long long)v[b] << (64 - KM_TAG_SHIFT)) >> (64 - KM_TAG_SHIFT);
    return (float)((double)a * (1.0 / FAISS_FXL));
}

// ---- faiss's k-means plan (host-built by ncn_kmeans_plan_fill, read by the kernel) ----
// 32-bit words: the header; init picks, uint16 [n_tri + 1][K] by point count nx (first K of
// rand_perm(seed + 1), through the subsample above the cap); training-set membership masks, one row
// of kmp_mask_row_words bits per point count above the subsampling cap K * FAISS_MAX_PTS
// (rand_perm(seed)'s first cap entries); split_clusters' FAISS_N_RAND floats.
enum { KMP_MAGIC = 0, KMP_N_TRI = 1, KMP_K = 2, KMP_CAP = 3, KMP_N_RAND = 4, KMP_INIT_OFF = 5, KMP_MASK_OFF = 6,
       KMP_RAND_OFF = 7, KMP_HEAD_WORDS = 8 };
constexpr uint32_t KMP_MAGIC_WORD = 0x4B4D5031u;
__host__ __device__ inline int kmp_mask_row_words(int n_tri) { return (n_tri + 31) >> 5; }
inline int64_t kmp_init_words(int n_tri, int K) { return ((int64_t)(n_tri + 1) * K + 1) / 2; }
inline int64_t kmp_mask_rows(int n_tri, int K) { return std::max<int64_t>(0, n_tri - (int64_t)K * FAISS_MAX_PTS); }
inline int64_t kmp_mask_off(int n_tri, int K) { return KMP_HEAD_WORDS + kmp_init_words(n_tri, K); }
inline int64_t kmp_rand_off(int n_tri, int K) {
    return kmp_mask_off(n_tri, K) + kmp_mask_rows(n_tri, K) * kmp_mask_row_words(n_tri);
}
inline int64_t kmp_words(int n_tri, int K) { return kmp_rand_off(n_tri, K) + FAISS_N_RAND; }
struct KmPlan {
    const uint32_t* p;
    __device__ __forceinline__ int n_tri() const { return (int)p[KMP_N_TRI]; }
    __device__ __forceinline__ int K() const { return (int)p[KMP_K]; }
    __device__ __forceinline__ int cap() const { return (int)p[KMP_CAP]; }
    __device__ __forceinline__ int n_rand() const { return (int)p[KMP_N_RAND]; }
    __device__ __forceinline__ int init(int nx, int k) const {
        return (int)((const uint16_t*)(p + p[KMP_INIT_OFF]))[(int64_t)nx * p[KMP_K] + k];
    }
    __device__ __forceinline__ bool member(int nx, int rank) const {
        if (nx <= cap()) return true;
        const int mw = kmp_mask_row_words(n_tri());
        return (p[p[KMP_MASK_OFF] + (int64_t)(nx - cap() - 1) * mw + (rank >> 5)] >> (rank & 31)) & 1u;
    }
    __device__ __forceinline__ const float* rnd() const { return (const float*)(p + p[KMP_RAND_OFF]); }
};

}  // namespace ncn
