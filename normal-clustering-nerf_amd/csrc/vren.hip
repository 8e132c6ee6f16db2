// Ray-AABB intersection, occupancy-grid ray marching, front-to-back compositing and the occupancy
// utilities for gfx950.  Replaces the reference `vren` kernels (models/csrc/intersection.cu,
// raymarching.cu, volumerendering.cu); every kernel cites the lines whose semantics it keeps.
//
// Floating-point contract: contraction is OFF for this whole file; the FMAs that the reference's
// nvcc build contracts (default --fmad=true) are written as explicit fmaf(), identically in the
// CPU oracle (oracle/vren_ref.c).  Division is IEEE (hipcc default correctly-rounded f32 div).
// This makes sample positions, voxel indices and sample counts bit-identical to the oracle.
//
// This file holds the launchers and the C ABI.  The device code, by stage:
//   vren_march.h         morton, mip, MarchConst, probe, skip; the serial walks (train and test)
//   vren_march_wave.h    the wave-parallel walk at constant dt; the fused marcher's walk launch
//   vren_march_pack.h    scan + pack (eager) and place (the fused marcher's second launch)
//   vren_aabb.h          the slab test of one box, ray_aabb_intersect
//   vren_composite.h     ray segments, CF_* and the long-ray dispatch; _fw.h / _bw.h: the compositors
//   vren_test_loop.h     the test compositor, compaction, the device-driven test loop
//   vren_util.h          morton / packbits kernels, count_samples, segment_csr
#pragma clang fp contract(off)

#include "common.h"
#include "../../include/ncnerf.h"
#include "vren_march.h"
#include "vren_march_wave.h"
#include "vren_march_pack.h"
#include "vren_aabb.h"
#include "vren_composite_fw.h"
#include "vren_composite_bw.h"
#include "vren_test_loop.h"
#include "vren_util.h"

using namespace ncn;

// ------------------------------------------------------------------------------------------------
// Launch helpers, then the C ABI
// Launches KERNEL<cascades == 1> (the marchers' ONE_CASCADE instance, or the general one) ...
#define NCN_LAUNCH_CASCADES(CASCADES, KERNEL, ...)                          \
    do {                                                                    \
        if ((CASCADES) == 1) hipLaunchKernelGGL(KERNEL<true>, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL<false>, __VA_ARGS__);                \
    } while (0)
// ... and KERNEL<cascades == 1, P> of the wave-parallel walk (P sub-windows per iteration).
#define NCN_LAUNCH_CASCADES_P(CASCADES, KERNEL, P, ...)                          \
    do {                                                                         \
        if ((CASCADES) == 1) hipLaunchKernelGGL((KERNEL<true, P>), __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<false, P>), __VA_ARGS__);                \
    } while (0)

// raymarching_test for ncn_march_test (ctrl NULL) and the device-driven loop (n_samples from ctrl).
static void launch_march_test(const float* rays_o, const float* rays_d, float* hits_t, const int64_t* alive,
                              int64_t n_alive, const uint8_t* bitfield, int cascades, float scale,
                              float exp_step_factor, int grid_size, int max_samples, int n_samples, float* xyzs,
                              float* dirs, float* deltas, float* ts, int32_t* n_eff, const int32_t* ctrl,
                              hipStream_t s) {
    NCN_LAUNCH_CASCADES(cascades, march_test_kernel, dim3(cdiv(n_alive, 64)), dim3(64), 0, s, rays_o, rays_d, hits_t,
                        alive, n_alive, bitfield, cascades, scale, exp_step_factor, grid_size, max_samples, n_samples,
                        xyzs, dirs, deltas, ts, n_eff, ctrl);
}

// composite_test_multi_fw for its three entries (offsets / ctrl NULL where the entry has none).
static void launch_composite_test(const float* sigmas, const float* raws, const float* deltas, const float* ts,
                                  int64_t* alive, int64_t n_alive, int n_samples, int n_rend, float T_threshold,
                                  const int32_t* n_eff, float* opacity, float* depth, float* rend,
                                  const int32_t* offsets, const int32_t* ctrl, hipStream_t s) {
    hipLaunchKernelGGL(composite_test_kernel, dim3(cdiv(n_alive, 256)), dim3(256), 0, s, sigmas, raws, deltas, ts,
                       alive, n_alive, n_samples, n_rend, T_threshold, n_eff, opacity, depth, rend, offsets, ctrl);
}

extern "C" {

int ncn_morton3D(const int32_t* coords, int64_t n, int32_t* out, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(morton3D_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, coords, n, out);
    NCN_LAUNCH_CHECK("ncn_morton3D");
    return 0;
}

int ncn_morton3D_invert(const int32_t* indices, int64_t n, int32_t* coords, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(morton3D_invert_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, indices, n,
                       coords);
    NCN_LAUNCH_CHECK("ncn_morton3D_invert");
    return 0;
}

int ncn_count_samples(const int64_t* total_samples, int64_t n_rays, const int32_t* counter, int64_t* sum_out,
                      double* acc, void* stream) {
    hipLaunchKernelGGL(count_samples_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, total_samples, n_rays,
                       counter, sum_out, acc);
    NCN_LAUNCH_CHECK("ncn_count_samples");
    return 0;
}

int ncn_segment_csr(const float* dL_dxyzs, const float* dL_ddirs, const float* ts, const int64_t* rays_a,
                    int64_t n_rays, float* dL_drays_o, float* dL_drays_d, void* stream) {
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(segment_csr_kernel, dim3(cdiv(n_rays, 4)), dim3(256), 0, (hipStream_t)stream, dL_dxyzs,
                       dL_ddirs, ts, rays_a, n_rays, dL_drays_o, dL_drays_d);
    NCN_LAUNCH_CHECK("ncn_segment_csr");
    return 0;
}

int ncn_packbits(const float* density_grid, int64_t n_bytes, float threshold, uint8_t* bitfield, void* stream) {
    if (n_bytes <= 0) return 0;
    NCN_REQUIRE(((uintptr_t)density_grid & 15) == 0, hipErrorInvalidValue, "ncn_packbits: grid must be 16B aligned");
    hipLaunchKernelGGL(packbits_kernel, dim3(cdiv(n_bytes, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)density_grid, n_bytes, threshold, bitfield);
    NCN_LAUNCH_CHECK("ncn_packbits");
    return 0;
}

int ncn_ray_aabb_intersect_near(const float* rays_o, const float* rays_d, int64_t n_rays, const float* centers,
                                const float* half_sizes, int64_t n_voxels, int max_hits, float near_distance,
                                int32_t* hit_cnt, float* hits_t, int64_t* hits_voxel_idx, void* stream) {
    if (n_rays <= 0) return 0;
    NCN_REQUIRE(max_hits >= 1 && max_hits <= 16, hipErrorInvalidValue,
                "ncn_ray_aabb_intersect: max_hits must be in [1,16] (got %d)", max_hits);
    dim3 g(cdiv(n_rays, 256)), b(256);
    hipStream_t s = (hipStream_t)stream;
    if (max_hits == 1)
        hipLaunchKernelGGL(ray_aabb_kernel<1>, g, b, 0, s, rays_o, rays_d, n_rays, centers, half_sizes, n_voxels,
                           max_hits, hit_cnt, hits_t, hits_voxel_idx, near_distance);
    else if (max_hits <= 4)
        hipLaunchKernelGGL(ray_aabb_kernel<4>, g, b, 0, s, rays_o, rays_d, n_rays, centers, half_sizes, n_voxels,
                           max_hits, hit_cnt, hits_t, hits_voxel_idx, near_distance);
    else
        hipLaunchKernelGGL(ray_aabb_kernel<16>, g, b, 0, s, rays_o, rays_d, n_rays, centers, half_sizes, n_voxels,
                           max_hits, hit_cnt, hits_t, hits_voxel_idx, near_distance);
    NCN_LAUNCH_CHECK("ncn_ray_aabb_intersect");
    return 0;
}

int ncn_ray_aabb_intersect(const float* rays_o, const float* rays_d, int64_t n_rays, const float* centers,
                           const float* half_sizes, int64_t n_voxels, int max_hits, int32_t* hit_cnt, float* hits_t,
                           int64_t* hits_voxel_idx, void* stream) {
    // near 0: no hit's t1 is in [0, 0), i.e. the plain reference kernel
    return ncn_ray_aabb_intersect_near(rays_o, rays_d, n_rays, centers, half_sizes, n_voxels, max_hits, 0.0f, hit_cnt,
                                       hits_t, hits_voxel_idx, stream);
}

int ncn_march_train_walk(const float* rays_o, const float* rays_d, const float* hits_t, const float* noise,
                         int64_t n_rays, const uint8_t* bitfield, int cascades, float scale, float exp_step_factor,
                         int grid_size, int max_samples, int32_t* counts, float* slab_xyz, float* slab_t,
                         float* slab_dt, void* stream) {
    if (n_rays <= 0) return 0;
    NCN_REQUIRE(cascades >= 1 && grid_size >= 1 && grid_size <= 1024 && max_samples >= 1, hipErrorInvalidValue,
                "ncn_march_train_walk: bad cascades/grid_size/max_samples");
    if (exp_step_factor == 0.0f) {  // constant dt: the wave-parallel walk
        dim3 g(cdiv(n_rays, 4)), b(256);
        NCN_LAUNCH_CASCADES_P(cascades, march_train_wave_kernel, 2, g, b, 0, (hipStream_t)stream, rays_o, rays_d,
                              hits_t, noise, n_rays, bitfield, cascades, scale, grid_size, max_samples, counts,
                              slab_xyz, slab_t, slab_dt);
        NCN_LAUNCH_CHECK("ncn_march_train_walk");
        return 0;
    }
    dim3 g(cdiv(n_rays, 64)), b(64);
    NCN_LAUNCH_CASCADES(cascades, march_train_walk_kernel, g, b, 0, (hipStream_t)stream, rays_o, rays_d, hits_t,
                        noise, n_rays, bitfield, cascades, scale, exp_step_factor, grid_size, max_samples, counts,
                        slab_xyz, slab_t, slab_dt);
    NCN_LAUNCH_CHECK("ncn_march_train_walk");
    return 0;
}

int64_t ncn_march_train_fused_work_bytes(int64_t n_rays) { return (n_rays + cdiv(n_rays, 4)) * 4; }

int ncn_march_train_fused(const float* rays_o, const float* rays_d, int64_t n_rays, float cx, float cy, float cz,
                          float hx, float hy, float hz, float near_distance, const float* noise, uint64_t seed,
                          const int64_t* rng_counter, const uint8_t* bitfield, int cascades, float scale,
                          int grid_size, int max_samples, float* slab_xyz, float* slab_t, float* slab_dt, void* work,
                          int64_t* rays_a, float* xyzs, float* dirs, float* deltas, float* ts, int32_t* counter,
                          void* stream) {
    if (n_rays <= 0) return 0;
    NCN_REQUIRE(cascades >= 1 && grid_size >= 1 && grid_size <= 1024 && max_samples >= 1 && work != nullptr,
                hipErrorInvalidValue, "ncn_march_train_fused: bad cascades/grid_size/max_samples/work");
    const int64_t nwg = cdiv(n_rays, 4);
    NCN_REQUIRE(nwg <= PLACE_MAX_WG && n_rays * (int64_t)max_samples < (1ll << 31) && max_samples < (1 << 24),
                hipErrorInvalidValue,
                "ncn_march_train_fused: n_rays must be <= %d (and n_rays * max_samples < 2^31)", 4 * PLACE_MAX_WG);
    int32_t* counts = (int32_t*)work;
    int32_t* wg_sum = counts + n_rays;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(nwg), b(256);
    NCN_LAUNCH_CASCADES_P(cascades, march_train_walk2_kernel, 2, g, b, 0, s, rays_o, rays_d, n_rays, cx, cy, cz, hx,
                          hy, hz, near_distance, noise, seed, rng_counter, bitfield, cascades, scale, grid_size,
                          max_samples, slab_xyz, slab_t, slab_dt, counts, wg_sum);
    NCN_LAUNCH_CHECK("ncn_march_train_fused(walk)");
    hipLaunchKernelGGL(march_train_place_kernel, g, b, 0, s, rays_d, n_rays, max_samples, counts, wg_sum, slab_xyz,
                       slab_t, slab_dt, rays_a, xyzs, dirs, deltas, ts, counter);
    NCN_LAUNCH_CHECK("ncn_march_train_fused(place)");
    return 0;
}

int ncn_march_train_scan(const int32_t* counts, int64_t n_rays, int64_t* rays_a, int32_t* counter, void* stream) {
    hipLaunchKernelGGL(march_train_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, n_rays, rays_a,
                       counter);
    NCN_LAUNCH_CHECK("ncn_march_train_scan");
    return 0;
}

int ncn_march_train_pack(const float* rays_d, const int64_t* rays_a, int64_t n_rays, int max_samples,
                         const float* slab_xyz, const float* slab_t, const float* slab_dt, float* xyzs, float* dirs,
                         float* deltas, float* ts, void* stream) {
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(march_train_pack_kernel, dim3(cdiv(n_rays, 4)), dim3(256), 0, (hipStream_t)stream, rays_d,
                       rays_a, n_rays, max_samples, slab_xyz, slab_t, slab_dt, xyzs, dirs, deltas, ts);
    NCN_LAUNCH_CHECK("ncn_march_train_pack");
    return 0;
}

int ncn_march_test(const float* rays_o, const float* rays_d, float* hits_t, const int64_t* alive, int64_t n_alive,
                   const uint8_t* bitfield, int cascades, float scale, float exp_step_factor, int grid_size,
                   int max_samples, int n_samples, float* xyzs, float* dirs, float* deltas, float* ts, int32_t* n_eff,
                   void* stream) {
    if (n_alive <= 0) return 0;
    NCN_REQUIRE(cascades >= 1 && grid_size >= 1 && n_samples >= 1, hipErrorInvalidValue, "ncn_march_test: bad args");
    launch_march_test(rays_o, rays_d, hits_t, alive, n_alive, bitfield, cascades, scale, exp_step_factor, grid_size,
                      max_samples, n_samples, xyzs, dirs, deltas, ts, n_eff, nullptr, (hipStream_t)stream);
    NCN_LAUNCH_CHECK("ncn_march_test");
    return 0;
}

// Workgroups for the long rays at the front of rays_a (the training step's rows put them first);
// the ones whose first row is short exit at once.
static int cf_coop_blocks(int64_t n_rays) { return (int)std::min<int64_t>(n_rays, 256); }

// KERNEL: a macro from the channel count to the kernel instance
#define NCN_DISPATCH_C(C_RT, KERNEL, ...)                                                       \
    switch (C_RT) {                                                                            \
        case 1: hipLaunchKernelGGL(KERNEL(1), __VA_ARGS__); break;                             \
        case 3: hipLaunchKernelGGL(KERNEL(3), __VA_ARGS__); break;                             \
        case 4: hipLaunchKernelGGL(KERNEL(4), __VA_ARGS__); break;                             \
        case 6: hipLaunchKernelGGL(KERNEL(6), __VA_ARGS__); break;                             \
        default: ncn::set_error("unsupported n_rend=%d (supported: 1,3,4,6)", C_RT);           \
                 return (int)hipErrorInvalidValue;                                             \
    }
#define NCN_FW_KERNEL(C) (composite_fw_kernel<C>)
#define NCN_BW_KERNEL(C) (composite_bw_kernel<C, false>)
#define NCN_BW_KERNEL_DWS(C) (composite_bw_kernel<C, true>)

int ncn_composite_train_fw_bg(const float* sigmas, const float* raws, const float* deltas, const float* ts,
                              const int64_t* rays_a, int64_t n_rays, int64_t n_samples, int n_rend, float T_threshold,
                              int64_t* total_samples, float* opacity, float* depth, float* rend, float* ws, float bg,
                              float* rgb_bg, void* stream) {
    if (n_rays <= 0) return 0;
    (void)n_samples;
    const int n_coop = cf_coop_blocks(n_rays);
    NCN_DISPATCH_C(n_rend, NCN_FW_KERNEL, dim3(n_coop + cdiv(n_rays, CF_WPB)), dim3(64 * CF_WPB), 0,
                   (hipStream_t)stream, sigmas, raws, deltas, ts, rays_a, n_rays, T_threshold, total_samples, opacity,
                   depth, rend, ws, bg, rgb_bg, n_coop);
    NCN_LAUNCH_CHECK("ncn_composite_train_fw");
    return 0;
}

int ncn_composite_train_fw(const float* sigmas, const float* raws, const float* deltas, const float* ts,
                           const int64_t* rays_a, int64_t n_rays, int64_t n_samples, int n_rend, float T_threshold,
                           int64_t* total_samples, float* opacity, float* depth, float* rend, float* ws,
                           void* stream) {
    return ncn_composite_train_fw_bg(sigmas, raws, deltas, ts, rays_a, n_rays, n_samples, n_rend, T_threshold,
                                     total_samples, opacity, depth, rend, ws, 0.f, nullptr, stream);
}

int ncn_composite_train_bw_bg(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb,
                              const float* dL_dws, const float* sigmas, const float* raws, const float* ws,
                              const float* deltas, const float* ts, const int64_t* rays_a, int64_t n_rays,
                              int64_t n_samples, int n_rend, const float* opacity, const float* depth,
                              const float* rend, float T_threshold, float bg, float* dL_dsigmas, float* dL_draws,
                              void* stream) {
    if (n_rays <= 0) return 0;
    (void)n_samples;
    const int n_coop = cf_coop_blocks(n_rays);
    const dim3 grid(n_coop + cdiv(n_rays, CF_WPB));
    if (dL_dws) {
        NCN_DISPATCH_C(n_rend, NCN_BW_KERNEL_DWS, grid, dim3(64 * CF_WPB), 0, (hipStream_t)stream, dL_dopacity,
                   dL_ddepth, dL_drgb, dL_dws, sigmas, raws, ws, deltas, ts, rays_a, n_rays, opacity, depth, rend,
                   T_threshold, dL_dsigmas, dL_draws, bg, n_coop);
    } else {
        NCN_DISPATCH_C(n_rend, NCN_BW_KERNEL, grid, dim3(64 * CF_WPB), 0, (hipStream_t)stream, dL_dopacity,
                   dL_ddepth, dL_drgb, dL_dws, sigmas, raws, ws, deltas, ts, rays_a, n_rays, opacity, depth, rend,
                   T_threshold, dL_dsigmas, dL_draws, bg, n_coop);
    }
    NCN_LAUNCH_CHECK("ncn_composite_train_bw");
    return 0;
}

int ncn_composite_train_bw(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drend,
                           const float* dL_dws, const float* sigmas, const float* raws, const float* ws,
                           const float* deltas, const float* ts, const int64_t* rays_a, int64_t n_rays,
                           int64_t n_samples, int n_rend, const float* opacity, const float* depth, const float* rend,
                           float T_threshold, float* dL_dsigmas, float* dL_draws, void* stream) {
    return ncn_composite_train_bw_bg(dL_dopacity, dL_ddepth, dL_drend, dL_dws, sigmas, raws, ws, deltas, ts, rays_a,
                                     n_rays, n_samples, n_rend, opacity, depth, rend, T_threshold, 0.f, dL_dsigmas,
                                     dL_draws, stream);
}

int ncn_composite_test_fw(const float* sigmas, const float* raws, const float* deltas, const float* ts,
                          int64_t* alive, int64_t n_alive, int n_samples, int n_rend, float T_threshold,
                          const int32_t* n_eff, float* opacity, float* depth, float* rend, void* stream) {
    if (n_alive <= 0) return 0;
    launch_composite_test(sigmas, raws, deltas, ts, alive, n_alive, n_samples, n_rend, T_threshold, n_eff, opacity,
                          depth, rend, nullptr, nullptr, (hipStream_t)stream);
    NCN_LAUNCH_CHECK("ncn_composite_test_fw");
    return 0;
}

int ncn_test_compact(const float* xyzs, const float* dirs, const int32_t* n_eff, int64_t n_alive, int n_samples,
                     int32_t* offsets, float* xyz_c, float* dir_c, int32_t* count, void* stream) {
    NCN_REQUIRE(n_alive >= 0 && n_samples >= 1 && n_alive * (int64_t)n_samples < (int64_t)INT32_MAX,
                hipErrorInvalidValue, "ncn_test_compact: n_alive * n_samples must fit int32");
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) {
        ncn::set_error("ncn_test_compact: memset failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    if (n_alive == 0) return 0;
    hipLaunchKernelGGL(test_compact_kernel, dim3(cdiv(n_alive, 256)), dim3(256), 0, (hipStream_t)stream, xyzs, dirs,
                       n_eff, n_alive, n_samples, offsets, xyz_c, dir_c, count);
    NCN_LAUNCH_CHECK("ncn_test_compact");
    return 0;
}

int ncn_composite_test_fw_compact(const float* sigmas_c, const float* raws_c, const int32_t* offsets,
                                  const float* deltas, const float* ts, int64_t* alive, int64_t n_alive,
                                  int n_samples, int n_rend, float T_threshold, const int32_t* n_eff, float* opacity,
                                  float* depth, float* rend, void* stream) {
    if (n_alive <= 0) return 0;
    NCN_REQUIRE(offsets != nullptr, hipErrorInvalidValue, "ncn_composite_test_fw_compact: offsets required");
    launch_composite_test(sigmas_c, raws_c, deltas, ts, alive, n_alive, n_samples, n_rend, T_threshold, n_eff, opacity,
                          depth, rend, offsets, nullptr, (hipStream_t)stream);
    NCN_LAUNCH_CHECK("ncn_composite_test_fw_compact");
    return 0;
}

int ncn_test_loop_march(const float* rays_o, const float* rays_d, float* hits_t, const int64_t* alive,
                        int64_t max_alive, const uint8_t* bitfield, int cascades, float scale, float exp_step_factor,
                        int grid_size, int max_samples, const int32_t* ctrl, float* xyzs, float* dirs, float* deltas,
                        float* ts, int32_t* n_eff, void* stream) {
    if (max_alive <= 0) return 0;
    NCN_REQUIRE(cascades >= 1 && grid_size >= 1 && ctrl, hipErrorInvalidValue, "ncn_test_loop_march: bad args");
    launch_march_test(rays_o, rays_d, hits_t, alive, max_alive, bitfield, cascades, scale, exp_step_factor, grid_size,
                      max_samples, 1, xyzs, dirs, deltas, ts, n_eff, ctrl, (hipStream_t)stream);
    NCN_LAUNCH_CHECK("ncn_test_loop_march");
    return 0;
}

int ncn_test_loop_index(const int32_t* n_eff, int64_t max_alive, int32_t* ctrl, int32_t* idx, void* stream) {
    if (max_alive <= 0) return 0;
    hipLaunchKernelGGL(test_index_kernel, dim3(TL_BLOCKS), dim3(256), 0, (hipStream_t)stream, n_eff, ctrl, idx);
    NCN_LAUNCH_CHECK("ncn_test_loop_index");
    return 0;
}

int ncn_test_loop_composite(const float* sigmas_c, const float* raws_c, const int32_t* offsets, const float* deltas,
                            const float* ts, int64_t* alive, int64_t max_alive, const int32_t* ctrl, int n_rend,
                            float T_threshold, const int32_t* n_eff, float* opacity, float* depth, float* rend,
                            void* stream) {
    if (max_alive <= 0) return 0;
    launch_composite_test(sigmas_c, raws_c, deltas, ts, alive, max_alive, 1, n_rend, T_threshold, n_eff, opacity,
                          depth, rend, offsets, ctrl, (hipStream_t)stream);
    NCN_LAUNCH_CHECK("ncn_test_loop_composite");
    return 0;
}

int ncn_test_loop_next(const int64_t* alive, int64_t* alive_next, int64_t max_alive, int32_t* ctrl,
                       int64_t* total_samples, int n_rays, int max_samples, int min_samples, void* stream) {
    if (max_alive <= 0) return 0;
    hipLaunchKernelGGL(test_alive_compact_kernel, dim3(TL_BLOCKS), dim3(256), 0, (hipStream_t)stream, alive,
                       alive_next, ctrl);
    hipLaunchKernelGGL(test_loop_next_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctrl, total_samples, n_rays,
                       max_samples, min_samples);
    NCN_LAUNCH_CHECK("ncn_test_loop_next");
    return 0;
}

}  // extern "C"
