// Normal-clustering loss path for gfx950: the launchers and the C ABI.  The device code, by stage:
//   loss_normals.h   normals from rendered depth over pixel triangles (datasets/hypersim_src/utils.py:504-541)
//   loss_photo.h     photometric MSE + opacity entropy, the fused backward of the reference configuration
//   cluster_ws.h, cluster_lloyd.h, cluster_select.h, cluster_kernel.h (arithmetic: kmeans_faiss.h)
//                    spherical k-means + Manhattan cluster selection + cluster losses and their analytic
//                    gradient (losses.py:47-166, 420-478) in ONE persistent launch of KM_BLOCKS = 16 workgroups:
//                    no device->host round trip (the reference copies the normals to the host for faiss, :434)
#pragma clang fp contract(off)

#include <atomic>
#include <cstring>
#include "common.h"
#include "../../include/ncnerf.h"
#include "loss_normals.h"
#include "loss_photo.h"
#include "cluster_kernel.h"

namespace ncn {

template <int K>
static void launch_cluster(const float* normals, int n_tri, int niter, const uint32_t* plan, float t_sim, float w_ort,
                           float w_dot, float w_l1, const float* w_dev, const int64_t* step_dev, float sched_start,
                           float sched_grow, const float* photo, float* out_losses, int32_t* out_labels,
                           float* out_centroids, float* dn, float* ws, hipStream_t s) {
    hipLaunchKernelGGL(cluster_kernel<K>, dim3(KM_BLOCKS), dim3(KM_THREADS), 0, s, normals, n_tri, niter, plan, t_sim,
                       w_ort, w_dot, w_l1, w_dev, step_dev, sched_start, sched_grow, photo, ws, out_losses, out_labels,
                       out_centroids, dn);
}

}  // namespace ncn

using namespace ncn;

extern "C" {

int64_t ncn_cluster_workspace_words(int K) { return km_ws_words(K); }
int64_t ncn_cluster_status_offset(int K) { return km_status_word(K); }

// ---- faiss k-means plan (host; layout in cluster_ws.h, draws in kmeans_faiss.h) ----
int64_t ncn_kmeans_plan_words(int n_tri, int K) {
    if (n_tri < 0 || K <= 0) return 0;
    return kmp_words(n_tri, K);
}

int ncn_kmeans_plan_fill(int n_tri, int K, uint32_t seed, uint32_t* out) {
    NCN_REQUIRE(out != nullptr && n_tri >= 0 && n_tri < 65536 && K > 0, hipErrorInvalidValue,
                "ncn_kmeans_plan_fill: bad arguments");
    const int cap = K * FAISS_MAX_PTS, mw = kmp_mask_row_words(n_tri);
    std::fill(out, out + kmp_words(n_tri, K), 0u);
    out[KMP_MAGIC] = KMP_MAGIC_WORD, out[KMP_N_TRI] = (uint32_t)n_tri, out[KMP_K] = (uint32_t)K;
    out[KMP_CAP] = (uint32_t)cap, out[KMP_N_RAND] = (uint32_t)FAISS_N_RAND, out[KMP_INIT_OFF] = KMP_HEAD_WORDS;
    out[KMP_MASK_OFF] = (uint32_t)kmp_mask_off(n_tri, K), out[KMP_RAND_OFF] = (uint32_t)kmp_rand_off(n_tri, K);
    uint16_t* init = (uint16_t*)(out + KMP_HEAD_WORDS);
    std::vector<int32_t> scratch;
    std::vector<int64_t> perm((size_t)std::max(cap, K)), perm1((size_t)K);
    faiss_rand_perm_prefix(std::max(cap, 1), seed + 1, K, perm1.data(), scratch);  // init picks of a subsampled training set
    for (int nx = K; nx <= n_tri; nx++) {
        if (nx == K) {  // faiss's nx == k corner case: the points themselves, in order
            for (int k = 0; k < K; k++) init[(int64_t)nx * K + k] = (uint16_t)k;
        } else if (nx <= cap) {
            faiss_rand_perm_prefix(nx, seed + 1, K, perm.data(), scratch);  // redo 0: seed + 1 + 0 * 15486557
            for (int k = 0; k < K; k++) init[(int64_t)nx * K + k] = (uint16_t)perm[k];
        } else {
            faiss_rand_perm_prefix(nx, seed, cap, perm.data(), scratch);  // subsample_training_set
            uint32_t* mask = out + kmp_mask_off(n_tri, K) + (int64_t)(nx - cap - 1) * mw;
            for (int i = 0; i < cap; i++) mask[perm[i] >> 5] |= 1u << (perm[i] & 31);
            for (int k = 0; k < K; k++) init[(int64_t)nx * K + k] = (uint16_t)perm[perm1[k]];
        }
    }
    std::vector<float> rnd(FAISS_N_RAND);
    faiss_rand_floats(1234u, FAISS_N_RAND, rnd.data());  // split_clusters: RandomGenerator rng(1234)
    memcpy(out + kmp_rand_off(n_tri, K), rnd.data(), sizeof(float) * FAISS_N_RAND);
    return 0;
}

int ncn_photo_loss_fwd(const float* rgb, const float* rgb_gt, const float* opacity, int64_t n_rays, float w_opacity,
                       float* loss, void* stream) {
    hipLaunchKernelGGL(photo_loss_fwd_kernel, dim3(1), dim3(PH_THREADS), 0, (hipStream_t)stream, rgb, rgb_gt, opacity,
                       n_rays, w_opacity, loss);
    NCN_LAUNCH_CHECK("ncn_photo_loss_fwd");
    return 0;
}

int ncn_photo_loss_bwd(const float* rgb, const float* rgb_gt, const float* opacity, int64_t n_rays, float w_opacity,
                       const float* loss, const float* upstream, float* dL_drgb, float* dL_dopacity, void* stream) {
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(photo_loss_bwd_kernel, dim3(cdiv(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, rgb, rgb_gt,
                       opacity, n_rays, w_opacity, loss, upstream, dL_drgb, dL_dopacity);
    NCN_LAUNCH_CHECK("ncn_photo_loss_bwd");
    return 0;
}

int ncn_photo_normals_count_fwd(const float* rgb, const float* rgb_gt, const float* opacity, int64_t n_rays,
                                float w_opacity, float* loss, const float* rays_o, const float* rays_d,
                                const float* depth, const int64_t* x1, const int64_t* x2, const int64_t* x3,
                                int64_t n_tri, float* normals, const int64_t* total_samples, int64_t n_count,
                                const int32_t* counter, int64_t* count_out, double* count_acc, void* stream) {
    NCN_REQUIRE(!total_samples || count_out, hipErrorInvalidValue, "ncn_photo_normals_count_fwd: count_out needed");
    const int nb0 = total_samples ? 2 : 1;
    hipLaunchKernelGGL(photo_normals_fwd_kernel, dim3(nb0 + cdiv(std::max<int64_t>(n_tri, 0), PH_THREADS)),
                       dim3(PH_THREADS), 0, (hipStream_t)stream, rgb, rgb_gt, opacity, n_rays, w_opacity, loss, rays_o,
                       rays_d, depth, x1, x2, x3, n_tri, normals, total_samples, n_count, counter, count_out,
                       count_acc);
    NCN_LAUNCH_CHECK("ncn_photo_normals_count_fwd");
    return 0;
}

int ncn_normals_fwd(const float* rays_o, const float* rays_d, const float* depth, const int64_t* x1, const int64_t* x2,
                    const int64_t* x3, int64_t n_tri, float* normals, void* stream) {
    if (n_tri <= 0) return 0;
    hipLaunchKernelGGL(normals_fwd_kernel, dim3(cdiv(n_tri, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d,
                       depth, x1, x2, x3, n_tri, normals);
    NCN_LAUNCH_CHECK("ncn_normals_fwd");
    return 0;
}

int ncn_normals_bwd(const float* rays_o, const float* rays_d, const float* depth, const int64_t* x1, const int64_t* x2,
                    const int64_t* x3, int64_t n_tri, const float* dL_dnormals, const float* term_weights,
                    float* dL_ddepth, void* stream) {
    if (n_tri <= 0) return 0;
    hipLaunchKernelGGL(normals_bwd_kernel, dim3(cdiv(n_tri, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d,
                       depth, x1, x2, x3, n_tri, dL_dnormals, term_weights, dL_ddepth);
    NCN_LAUNCH_CHECK("ncn_normals_bwd");
    return 0;
}

int ncn_normals_bwd_rays(const float* rays_o, const float* rays_d, const float* depth, const int64_t* x1,
                         const int64_t* x2, const int64_t* x3, int64_t n_tri, const float* dL_dnormals,
                         const float* term_weights, float* dL_ddepth, float* dL_drays_o, float* dL_drays_d,
                         void* stream) {
    if (n_tri <= 0) return 0;
    NCN_REQUIRE(dL_ddepth && dL_drays_o && dL_drays_d, hipErrorInvalidValue,
                "ncn_normals_bwd_rays: dL_ddepth, dL_drays_o and dL_drays_d required");
    hipLaunchKernelGGL(normals_bwd_rays_kernel, dim3(cdiv(n_tri, 256)), dim3(256), 0, (hipStream_t)stream, rays_o,
                       rays_d, depth, x1, x2, x3, n_tri, dL_dnormals, term_weights, dL_ddepth, dL_drays_o, dL_drays_d);
    NCN_LAUNCH_CHECK("ncn_normals_bwd_rays");
    return 0;
}

int ncn_nerf_loss_bwd(const float* rgb, const float* rgb_gt, const float* opacity, int64_t n_rays, float w_opacity,
                      const float* photo_loss, const float* rays_o, const float* rays_d, const float* depth,
                      const float* dL_dnormals, const float* up_total, const float* up_terms, float* dL_drgb,
                      float* dL_dopacity, float* dL_ddepth, void* stream) {
    NCN_REQUIRE(n_rays % 64 == 0, hipErrorInvalidValue, "ncn_nerf_loss_bwd: n_rays=%lld is not whole 8x8 patches",
                (long long)n_rays);
    NCN_REQUIRE((dL_drgb == nullptr) == (dL_dopacity == nullptr), hipErrorInvalidValue,
                "ncn_nerf_loss_bwd: dL_drgb and dL_dopacity are written together (both or neither)");
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(nerf_loss_bwd_kernel, dim3(cdiv(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, rgb, rgb_gt,
                       opacity, n_rays, w_opacity, photo_loss, rays_o, rays_d, depth, dL_dnormals, up_total, up_terms,
                       dL_drgb, dL_dopacity, dL_ddepth);
    NCN_LAUNCH_CHECK("ncn_nerf_loss_bwd");
    return 0;
}

#ifdef NCN_DIAG_CL_TIMES
int ncn_diag_cl_times(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(ncn_cl_times), sizeof(unsigned long long) * 64);
}
#endif

// Co-residency of the clustering kernel's KM_BLOCKS workgroups (they meet at grid barriers and
// poll each other's partials, so all of them must be resident at once): per-CU occupancy of the
// kernel (registers, LDS, waves) x the CUs left free by `busy_cus` CUs that concurrent work can
// hold entirely (the split step's rgb pass: one workgroup per CU, its LDS takes the CU).
int ncn_cluster_coresidency(int K, int busy_cus, int* capacity) {
    NCN_REQUIRE(K == 10 || K == 20, hipErrorInvalidValue, "ncn_cluster_coresidency: K must be 10 or 20 (got %d)", K);
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess)
        e = K == 20 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cluster_kernel<20>, KM_THREADS, 0)
                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cluster_kernel<10>, KM_THREADS, 0);
    NCN_REQUIRE(e == hipSuccess, e, "ncn_cluster_coresidency: device query failed (%s)", hipGetErrorString(e));
    const int cap = std::max(0, cus - std::max(0, busy_cus)) * per_cu;
    if (capacity) *capacity = cap;
    NCN_REQUIRE(cap >= KM_BLOCKS, hipErrorCooperativeLaunchTooLarge,
                "ncn_cluster_coresidency: the clustering's %d workgroups cannot all be resident: %d CUs - %d busy "
                "= %d free x %d workgroups per CU = %d", KM_BLOCKS, cus, busy_cus, std::max(0, cus - busy_cus), per_cu,
                cap);
    return 0;
}

int ncn_cluster_loss(const float* normals, int64_t n_tri, int K, int niter, const uint32_t* kmeans_plan, float t_similar,
                     float w_ort, float w_dot, float w_l1, const float* w_dev, const int64_t* step_dev,
                     float sched_start, float sched_grow, const float* photo_loss, float* out_losses,
                     int32_t* out_labels, float* out_centroids, float* dL_dnormals, float* workspace,
                     void* stream) {
    NCN_REQUIRE(n_tri >= 0 && n_tri <= CL_MAX_TRI, hipErrorInvalidValue,
                "ncn_cluster_loss: n_tri=%lld exceeds %d", (long long)n_tri, CL_MAX_TRI);
    // refuse (rather than spin into the barrier timeout) on a device that cannot hold the workgroups
    // at all; checked once per (device, K) — the answer depends on the device and on the kernel
    // instance (K sets its LDS) — and cached in an atomic (0 unknown, 1 resident, 2 refused; a racing
    // first call computes the same answer twice)
    static std::atomic<int> coresident[NCN_MAX_DEVICES][2];
    int dev = 0;
    NCN_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < NCN_MAX_DEVICES, hipErrorInvalidDevice,
                "ncn_cluster_loss: current device %d out of range", dev);
    if (K == 10 || K == 20) {
        std::atomic<int>& c = coresident[dev][K == 20];
        int v = c.load(std::memory_order_relaxed);
        if (v == 0) {
            v = ncn_cluster_coresidency(K, 0, nullptr) == 0 ? 1 : 2;
            c.store(v, std::memory_order_relaxed);
        }
        NCN_REQUIRE(v == 1, hipErrorCooperativeLaunchTooLarge,
                    "ncn_cluster_loss: the device cannot hold the clustering's %d co-resident workgroups", KM_BLOCKS);
    }
    NCN_REQUIRE(niter >= 0 && niter <= 30, hipErrorInvalidValue, "ncn_cluster_loss: niter must be in [0, 30]");
    NCN_REQUIRE(kmeans_plan != nullptr, hipErrorInvalidValue, "ncn_cluster_loss: kmeans_plan required (ncn_kmeans_plan_fill)");
    NCN_REQUIRE(K == 10 || K == 20, hipErrorInvalidValue, "ncn_cluster_loss: K must be 10 or 20 (got %d)", K);
    (K == 20 ? launch_cluster<20> : launch_cluster<10>)(
        normals, (int)n_tri, niter, kmeans_plan, t_similar, w_ort, w_dot, w_l1, w_dev, step_dev, sched_start, sched_grow,
        photo_loss, out_losses, out_labels, out_centroids, dL_dnormals, workspace, (hipStream_t)stream);
    NCN_LAUNCH_CHECK("ncn_cluster_loss");
    return 0;
}

}  // extern "C"
