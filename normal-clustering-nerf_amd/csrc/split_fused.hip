// The split training step's loss node in two launches on one stream (ncn_split_loss_fused), so that
// the stretch between the compositor forward and the joint compositor backward crosses no queue:
//   1. photo_normals_draws_kernel: the workgroups of photo_normals_fwd_kernel (loss_photo.h) and,
//      behind them, the rgb-only compositor backward (vren_composite_bw.h with the dL/dsigma terms
//      compiled out): dL/draws = w * dL/drgb of the photometric term, one wave per row of rays_a.
//      It runs while the one-workgroup photometric reduction leaves the device idle.
//   2. cluster_rgb_kernel: workgroups [0, KM_BLOCKS) are the clustering (cluster_kernel.h), the rest
//      the rgb part of the field's MLP backward (field_bwd_mlp.h), which no longer waits on a side
//      stream beside it.  Neither role reads, polls or waits on anything the other writes.
// The stages keep the floating-point contraction of their own translation units (loss.hip and
// vren.hip: off; field.hip: the compiler's default), so every value is bit for bit what the
// separate launches give.
#pragma clang fp contract(off)
#include <algorithm>
#include <atomic>
#include "common.h"
#include "../../include/ncnerf.h"
#include "loss_normals.h"
#include "loss_photo.h"
#include "vren_composite_bw.h"
#include "cluster_kernel.h"
#pragma clang fp contract(fast)
#include "field_bwd_mlp.h"
#pragma clang fp contract(off)

namespace ncn {

// ---- launch 1 ----
// Workgroups [0, nb_fwd): photo_normals_fwd_kernel's.  Then n_coop workgroups for the long rays at
// the front of rays_a (their first CF_WPB waves take a ray as composite_bw_kernel's workgroups do;
// the other waves leave at once, and a wave that has ended does not count at the barrier), then
// one wave per row, DR_WPB rows per workgroup.  dL/drgb of a ray is nerf_loss_bwd_kernel's expression
// for up_terms = NULL with the validity flag taken as 1: the flag (photo[2]) is written by
// workgroup 0 of this same launch, so the consumer of dL_draws applies it (field_bwd_body's rgb_on).
constexpr int DR_WPB = PH_THREADS / 64;
__global__ __launch_bounds__(PH_THREADS) void photo_normals_draws_kernel(
    const float* __restrict__ rgb, const float* __restrict__ gt, const float* __restrict__ op, int64_t R, float w_op,
    float* __restrict__ loss, const float* __restrict__ o, const float* __restrict__ d,
    const float* __restrict__ depth, const int64_t* __restrict__ x1, const int64_t* __restrict__ x2,
    const int64_t* __restrict__ x3, int64_t T, float* __restrict__ normals, const int64_t* __restrict__ cnt_total,
    int64_t cnt_n, const int32_t* __restrict__ cnt_counter, int64_t* __restrict__ cnt_out, double* __restrict__ cnt_acc,
    int nb_fwd, const float* __restrict__ up_total, const float* __restrict__ sigmas, const float* __restrict__ deltas,
    const int64_t* __restrict__ rays_a, float T_thr, float* __restrict__ dL_draws, int n_coop) {
    if ((int)blockIdx.x < nb_fwd) {
        photo_normals_fwd_wg((int)blockIdx.x, rgb, gt, op, R, w_op, loss, o, d, depth, x1, x2, x3, T, normals, cnt_total,
                             cnt_n, cnt_counter, cnt_out, cnt_acc);
        return;
    }
    const int b = (int)blockIdx.x - nb_fwd, wv = threadIdx.x >> 6;
    const float ga = (up_total ? *up_total : 0.f) + 0.f;  // u[0] of nerf_loss_bwd_kernel
    const float sa = 2.f / (float)(3 * R);
    float dR[3];
    if (b < n_coop) {
        if (wv >= CF_WPB) return;
        for (int64_t row = b; cf_long_row(rays_a, R, row); row += n_coop) {
            const int64_t ray = rays_a[3 * row];
#pragma unroll
            for (int c = 0; c < 3; c++) dR[c] = photo_drgb(ga, sa, rgb[3 * ray + c], gt[3 * ray + c]);
            composite_bw_coop<3, false, false>(nullptr, nullptr, dR, nullptr, sigmas, nullptr, nullptr, deltas, nullptr,
                                               rays_a, row, nullptr, nullptr, nullptr, T_thr, nullptr, dL_draws, 0.f);
        }
        return;
    }
    const int64_t row = __builtin_amdgcn_readfirstlane((b - n_coop) * DR_WPB + wv);
    if (row >= R) return;  // (wave-uniform: the surplus waves of the last workgroup)
    RaySeg g;
    g.ray = rays_a[3 * row];
    g.start = rays_a[3 * row + 1];
    g.N = (int)rays_a[3 * row + 2];
    g.live = true;
    if (g.N > CF_LONG && g.N <= CF_COOP_MAX && cf_coop_takes(rays_a, row, n_coop)) return;  // a workgroup has it
#pragma unroll
    for (int c = 0; c < 3; c++) dR[c] = photo_drgb(ga, sa, rgb[3 * g.ray + c], gt[3 * g.ray + c]);
    composite_bw_ray<3, false, false>(nullptr, nullptr, dR, nullptr, sigmas, nullptr, nullptr, deltas, nullptr, g, nullptr,
                                      nullptr, nullptr, T_thr, nullptr, dL_draws, 0.f);
}

// ---- launch 2 ----
struct ClusterArgs {
    const float* normals;
    int n_tri, niter;
    const uint32_t* plan;
    float t_sim, w_ort, w_dot, w_l1;
    const float* w_dev;
    const int64_t* step_dev;
    float sched_start, sched_grow;
    const float* photo;
    float* ws;
    float* out_losses;
    int32_t* out_labels;
    float* out_centroids;
    float* dn;
};
struct RgbArgs {
    const float* dirs;
    int64_t n;
    const int32_t* n_dev;
    const uint16_t* wpacked;
    const void* enc;
    const float* dL_drgb;
    const float* loss_scale;
    float* dE_ws;
    float* slab;
    float* level_max;
    const int32_t* order;
    float* stash;
    const float* xyzs;
};

static_assert(KM_THREADS == BWD_THREADS, "the two roles share one workgroup shape");
// One LDS arena of the larger role's need: the rgb pass's 158 KB, so every workgroup owns a CU, as a
// clustering workgroup beside the rgb pass does in the forked step.
template <int K, typename T>
constexpr size_t fused_lds_bytes() {
    return sizeof(ClusterLds<K>) > sizeof(BwdLds<T, BWD_RGB>) ? sizeof(ClusterLds<K>) : sizeof(BwdLds<T, BWD_RGB>);
}
template <int K, typename T>
__global__ __launch_bounds__(BWD_THREADS, 2) void cluster_rgb_kernel(const ClusterArgs c, const RgbArgs r) {
    __shared__ __attribute__((aligned(16))) unsigned char arena[fused_lds_bytes<K, T>()];
    if (blockIdx.x < KM_BLOCKS) {
        cluster_body<K>(*reinterpret_cast<ClusterLds<K>*>(arena), (int)blockIdx.x, c.normals, c.n_tri, c.niter, c.plan,
                        c.t_sim, c.w_ort, c.w_dot, c.w_l1, c.w_dev, c.step_dev, c.sched_start, c.sched_grow, c.photo, c.ws,
                        c.out_losses, c.out_labels, c.out_centroids, c.dn);
    } else {
        // photo[2]: the photometric term's validity flag, left out of launch 1's dL_draws
        BwdLds<T, BWD_RGB>& l = *reinterpret_cast<BwdLds<T, BWD_RGB>*>(arena);
        field_bwd_body<T, BWD_RGB, false>(l.F32s, l.F16s, l.X, (int)blockIdx.x - KM_BLOCKS,
                                          (int)gridDim.x - KM_BLOCKS, c.photo + 2, r.dirs, r.n, r.n_dev, r.wpacked,
                                          (const typename Mfma<T>::v8*)r.enc, nullptr, r.dL_drgb, r.loss_scale, r.dE_ws,
                                          r.slab, r.level_max, r.order, nullptr, r.stash, r.xyzs, nullptr, nullptr);
    }
}

template <int K, typename T>
static hipError_t fused_per_cu(int* per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, cluster_rgb_kernel<K, T>, BWD_THREADS, 0);
}
template <int K, typename T>
static void launch_fused(int grid, hipStream_t s, const ClusterArgs& c, const RgbArgs& r) {
    hipLaunchKernelGGL((cluster_rgb_kernel<K, T>), dim3(grid), dim3(BWD_THREADS), 0, s, c, r);
}

}  // namespace ncn

using namespace ncn;

extern "C" {

int ncn_split_loss_fused(const float* rgb, const float* rgb_gt, const float* opacity, int64_t n_rays, float w_opacity,
                         float* photo_loss, const float* rays_o, const float* rays_d, const float* depth,
                         const int64_t* x1, const int64_t* x2, const int64_t* x3, int64_t n_tri, float* normals,
                         const int64_t* total_samples, const int32_t* counter, int64_t* count_out, double* count_acc,
                         const float* up_total, const float* sigmas, const float* deltas, const int64_t* rays_a,
                         float T_threshold, float* dL_draws, int K, int niter, const uint32_t* kmeans_plan,
                         float t_similar, float w_ort, float w_dot, float w_l1, const float* w_dev,
                         const int64_t* step_dev, float sched_start, float sched_grow, float* out_losses,
                         int32_t* out_labels, float* out_centroids, float* dL_dnormals, float* workspace,
                         const float* xyzs, const float* dirs, int64_t n, const int32_t* n_dev, const int32_t* order,
                         const uint16_t* weights_packed, int precision, const uint16_t* enc_cache,
                         const float* loss_scale, int n_blocks, float* slab, float* dE_ws, float* level_max,
                         float* dh_stash, void* stream) {
    NCN_REQUIRE(K == 10 || K == 20, hipErrorInvalidValue, "ncn_split_loss_fused: K must be 10 or 20 (got %d)", K);
    NCN_REQUIRE(precision == NCN_PREC_F16 || precision == NCN_PREC_BF16, hipErrorInvalidValue,
                "ncn_split_loss_fused: precision must be NCN_PREC_F16 or NCN_PREC_BF16");
    NCN_REQUIRE(n_blocks >= 0, hipErrorInvalidValue, "ncn_split_loss_fused: n_blocks must not be negative");
    // Co-residency by count: the clustering's workgroups meet at grid barriers, and a workgroup of
    // this kernel takes a whole CU's LDS, so all KM_BLOCKS + n_blocks must fit the device at once.
    // The capacity (CUs x workgroups per CU of the kernel instance) is cached per (device, K, operand).
    static std::atomic<int> capacity[NCN_MAX_DEVICES][2][2];
    int dev = 0;
    NCN_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < NCN_MAX_DEVICES, hipErrorInvalidDevice,
                "ncn_split_loss_fused: current device %d out of range", dev);
    const bool k20 = K == 20, bf = precision == NCN_PREC_BF16;
    int cap = capacity[dev][k20][bf].load(std::memory_order_relaxed);
    if (cap == 0) {
        int cus = 0, per_cu = 0;
        hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e == hipSuccess)
            e = k20 ? (bf ? fused_per_cu<20, __bf16>(&per_cu) : fused_per_cu<20, _Float16>(&per_cu))
                    : (bf ? fused_per_cu<10, __bf16>(&per_cu) : fused_per_cu<10, _Float16>(&per_cu));
        NCN_REQUIRE(e == hipSuccess, e, "ncn_split_loss_fused: device query failed (%s)", hipGetErrorString(e));
        cap = std::max(1, cus * per_cu);
        capacity[dev][k20][bf].store(cap, std::memory_order_relaxed);
    }
    const int nb_cap = n > 0 ? bwd_blocks_of(n) : 0, nb_rgb = n_blocks > 0 ? std::min(n_blocks, nb_cap) : nb_cap;
    // (refused on the requested count too, so that a caller can check its cap with n_rays = 0 before capturing)
    NCN_REQUIRE(KM_BLOCKS + std::max(n_blocks, nb_rgb) <= cap, hipErrorCooperativeLaunchTooLarge,
                "ncn_split_loss_fused: the clustering's %d workgroups and %d of the rgb pass cannot all be resident: "
                "the device holds %d workgroups of the fused kernel", KM_BLOCKS, std::max(n_blocks, nb_rgb), cap);
    if (n_rays <= 0) return 0;
    NCN_REQUIRE(n_rays % 64 == 0 && n_tri == (n_rays / 64) * 49, hipErrorInvalidValue,
                "ncn_split_loss_fused: n_rays=%lld must be whole 8x8 patches and n_tri=%lld their triangles",
                (long long)n_rays, (long long)n_tri);
    NCN_REQUIRE(n_tri <= CL_MAX_TRI, hipErrorInvalidValue, "ncn_split_loss_fused: n_tri=%lld exceeds %d",
                (long long)n_tri, CL_MAX_TRI);
    NCN_REQUIRE(niter >= 0 && niter <= 30, hipErrorInvalidValue, "ncn_split_loss_fused: niter must be in [0, 30]");
    NCN_REQUIRE(kmeans_plan != nullptr, hipErrorInvalidValue, "ncn_split_loss_fused: kmeans_plan required (ncn_kmeans_plan_fill)");
    NCN_REQUIRE(!total_samples || count_out, hipErrorInvalidValue, "ncn_split_loss_fused: count_out needed");
    NCN_REQUIRE(n <= 0 || (level_max && dh_stash && dL_draws), hipErrorInvalidValue,
                "ncn_split_loss_fused: level_max, dh_stash and dL_draws required");
    NCN_REQUIRE((((uintptr_t)dE_ws | (uintptr_t)enc_cache | (uintptr_t)weights_packed | (uintptr_t)dh_stash) & 15) == 0,
                hipErrorInvalidValue, "ncn_split_loss_fused: dE_ws / enc_cache / weights_packed / dh_stash must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const int nb_fwd = (total_samples ? 2 : 1) + (int)cdiv(n_tri, PH_THREADS);
    const int n_coop = (int)std::min<int64_t>(n_rays, 256);  // (the compositor backward's, vren.hip cf_coop_blocks)
    hipLaunchKernelGGL(photo_normals_draws_kernel, dim3(nb_fwd + n_coop + (int)cdiv(n_rays, DR_WPB)), dim3(PH_THREADS), 0,
                       s, rgb, rgb_gt, opacity, n_rays, w_opacity, photo_loss, rays_o, rays_d, depth, x1, x2, x3, n_tri,
                       normals, total_samples, n_rays, counter, count_out, count_acc, nb_fwd, up_total, sigmas, deltas,
                       rays_a, T_threshold, dL_draws, n_coop);
    NCN_LAUNCH_CHECK("ncn_split_loss_fused (photo, normals, draws)");
    const ClusterArgs c = {normals, (int)n_tri, niter, kmeans_plan, t_similar, w_ort, w_dot, w_l1, w_dev, step_dev,
                           sched_start, sched_grow, photo_loss, workspace, out_losses, out_labels, out_centroids,
                           dL_dnormals};
    const RgbArgs r = {dirs, n, n_dev, weights_packed, enc_cache, dL_draws, loss_scale, dE_ws, slab, level_max, order,
                       dh_stash, xyzs};
    const auto launch = k20 ? (bf ? launch_fused<20, __bf16> : launch_fused<20, _Float16>)
                            : (bf ? launch_fused<10, __bf16> : launch_fused<10, _Float16>);
    launch(KM_BLOCKS + nb_rgb, s, c, r);
    NCN_LAUNCH_CHECK("ncn_split_loss_fused (clustering, rgb pass)");
    return 0;
}

}  // extern "C"
