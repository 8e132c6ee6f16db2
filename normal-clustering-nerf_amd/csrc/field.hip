// NGPMT field for gfx950: multires hash-grid encoding (tiny-cuda-nn Grid/Hash semantics) fused
// with sigma_net (32->64->16), TruncExp, and rgb_net, replacing tcnn Encoding + two FullyFusedMLPs
// (reference models/ngp_mt.py:70-113, 157-229) and TruncExp (models/custom_functions.py:162-173).
// rgb_net is tcnn's network as built by the reference: `tcnn.Network(n_input_dims=19, ...)` wraps
// an Identity encoding that pads the 19 inputs cat[d/|d|, h] to the FullyFusedMLP's 16-alignment
// (32) with the value 1.0 (a learned bias in the padded columns), and pads the 3 outputs to 16:
// W3 is 64x32, W5 16x64 (rgb_net.params = 7168, sigma_net.params = 3072, as tcnn).
//
// Layout ("transposed activations"): every layer is computed as  Y^T = W . X^T  with the gfx950
// v_mfma_f32_16x16x32_{f16,bf16} (K = 32 per instruction), samples on the MFMA column (lane & 15),
// features on the rows.  The accumulator of a layer (lane (g,r) holds rows 4g..4g+3 of column r)
// is the B operand of the next layer with no data movement: two 16-row accumulator tiles side by
// side form a K = 32 operand whose element j of lane group g is feature phi(g,j) = 4g+j (j < 4, the
// first tile) or 16+4g+j-4 (the second), and the A fragments (weights) are packed in the same
// permuted K order.  A wave owns 16 samples per step; lane (g,r) encodes hash levels
// {2g, 2g+1, 8+2g, 9+2g} of sample r — exactly features phi(g, 0..7) of the encoding, i.e. the
// layer-1 B operand — and in the backward scatters the gradient of those levels.  Weights live in
// LDS as pre-packed MFMA fragments (ncn_field_pack_weights, 16 B per lane per K=32 fragment).
// Operand precision is a template parameter: fp16 (tcnn's FullyFusedMLP precision) or bf16
// (config #3); fp32 hash table + fp32 trilinear interpolation, fp32 accumulation either way.
// One translation unit on purpose: the device code is in the field_*.h headers, one per stage (DESIGN.md,
// source map), and this file holds the launchers and the C ABI.  (One instantiation of the MLP backward
// lives beside it, in field_rgb_din.hip, which says why; field_bwd_launch.h is what the two share.)
#include <algorithm>
#include <cstring>
#include "field_fwd.h"
#include "field_bwd_mlp.h"
#include "field_bwd_launch.h"
#include "field_scatter.h"
#include "field_bwd_dx.h"

namespace ncn {
static int scatter_grid(int64_t n_cap) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(256 * 1024 / SC_THREADS, (n_cap + 255) / 256));  // 1024 threads per CU
}

static LevelTable make_table(const uint32_t* levels) {
    LevelTable t;
    for (int l = 0; l < 16; l++) {
        memcpy(&t.scale[l], &levels[4 * l], 4);
        t.res[l] = levels[4 * l + 1];
        t.params[l] = levels[4 * l + 2];
        t.offset[l] = levels[4 * l + 3];
    }
    return t;
}

constexpr int64_t NCN_FWD_MAX_BLOCKS = 4096;  // (round 5: 1792 / 2048 / 8192 blocks measured the same, 84-85 us)
static int fwd_grid(int64_t n) {
    const int64_t groups = (n + 15) / 16;
    const int64_t g = std::min<int64_t>(std::max<int64_t>((groups + 3) / 4, 1), NCN_FWD_MAX_BLOCKS);
    return (int)((g + 7) & ~(int64_t)7);  // a multiple of 8 (xcd_block)
}
}  // namespace ncn
using namespace ncn;

static const char* xyzs_unaligned(const float* xyzs) {
    return ((uintptr_t)xyzs & 15) == 0 ? nullptr : "xyzs must be 16-byte aligned";
}

// (ncn_field_reduce_wgrad / _parts; `name` for the launch check's message)
static int reduce_wgrad(const char* name, const float* slab, int nb_sigma, int nb_rgb, float* grad_w, void* stream) {
    const int nb = std::max(nb_sigma, nb_rgb);
    if (nb <= 0) return 0;
    hipLaunchKernelGGL(reduce_wgrad_kernel, dim3(cdiv(NCN_FIELD_NW, 256), cdiv(nb, WRED_CHUNK)), dim3(256), 0,
                       (hipStream_t)stream, slab, nb_sigma, nb_rgb, grad_w);
    NCN_LAUNCH_CHECK(name);
    return 0;
}

extern "C" {
int ncn_field_pack_map(int32_t* src_index, void* stream) {
    hipLaunchKernelGGL(pack_map_kernel, dim3(N_FRAG32 + N_FRAG16), dim3(64), 0, (hipStream_t)stream, src_index);
    NCN_LAUNCH_CHECK("ncn_field_pack_map");
    return 0;
}

int ncn_field_pack_weights(const float* w_master, uint16_t* weights_packed, int precision, void* stream) {
    NCN_REQUIRE(precision == NCN_PREC_F16 || precision == NCN_PREC_BF16, hipErrorInvalidValue,
                "ncn_field_pack_weights: precision must be NCN_PREC_F16 or NCN_PREC_BF16");
    with_operand(precision, [&](auto op) {
        typedef typename decltype(op)::type T;
        hipLaunchKernelGGL(pack_weights_kernel<T>, dim3(N_FRAG32 + N_FRAG16), dim3(64), 0, (hipStream_t)stream, w_master,
                           (T*)weights_packed);
    });
    NCN_LAUNCH_CHECK("ncn_field_pack_weights");
    return 0;
}

// `levels` is a HOST array of 16 x {scale f32 bits, resolution, params, offset}.
int ncn_field_sort_windows(const float* xyzs, int64_t n, const int32_t* n_dev, float xyz_min, float xyz_extent,
                           int32_t* order, void* stream) {
    if (n <= 0) return 0;
    NCN_REQUIRE(xyz_extent > 0.f, hipErrorInvalidValue, "ncn_field_sort_windows: xyz_extent must be positive");
    hipLaunchKernelGGL(sort_windows_kernel, dim3((unsigned)cdiv(n, SORT_W)), dim3(SORT_THREADS), 0, (hipStream_t)stream,
                       xyzs, n, n_dev, xyz_min, 1.0f / xyz_extent, order);
    NCN_LAUNCH_CHECK("ncn_field_sort_windows");
    return 0;
}

int ncn_field_fwd(const float* xyzs, const float* dirs, int64_t n, const int32_t* n_dev, const int32_t* order,
                  const float* table, const uint32_t* levels, float xyz_min, float xyz_extent,
                  const uint16_t* weights_packed, int precision, int mode, float* sigmas, float* rgbs,
                  uint16_t* enc_cache, void* stream) {
    if (n <= 0) return 0;
    NCN_REQUIRE(mode >= 0 && mode <= 2, hipErrorInvalidValue, "ncn_field_fwd: mode must be 0, 1 or 2");
    NCN_REQUIRE(mode != 2 || (enc_cache && !order), hipErrorInvalidValue,
                "ncn_field_fwd: mode 2 needs enc_cache (scratch) and no processing order");
    NCN_REQUIRE(precision == NCN_PREC_F16 || precision == NCN_PREC_BF16, hipErrorInvalidValue,
                "ncn_field_fwd: precision must be NCN_PREC_F16 or NCN_PREC_BF16");
    NCN_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)enc_cache & 15) == 0 && ((uintptr_t)weights_packed & 15) == 0,
                hipErrorInvalidValue, "ncn_field_fwd: table 8-byte, enc_cache / weights_packed 16-byte aligned");
    const LevelTable Lt = make_table(levels);
    if (mode == 2) {  // level-split encoding over the XCDs first (n = capacity; n_dev = the count)
        NCN_REQUIRE(n <= (int64_t)INT32_MAX * 256 / 16, hipErrorInvalidValue, "ncn_field_fwd: n too large");
        const int nb = (int)((n + 255) / 256);
        with_operand(precision, [&](auto op) {
            typedef typename decltype(op)::type T;
            hipLaunchKernelGGL(encode_xcd_kernel<T>, dim3(16 * nb), dim3(256), 0, (hipStream_t)stream, xyzs, n, n_dev,
                               (const float2*)table, Lt, xyz_min, xyz_extent, nb, (T*)enc_cache);
        });
        NCN_LAUNCH_CHECK("ncn_field_fwd (encode)");
    }
    with_operand(precision, [&](auto op) {
        typedef typename decltype(op)::type T;
        typedef typename Mfma<T>::v8 v8;
        hipLaunchKernelGGL((mode == 2 ? field_fwd_kernel<T, true> : field_fwd_kernel<T, false>), dim3(fwd_grid(n)),
                           dim3(256), 0, (hipStream_t)stream, xyzs, dirs, n, n_dev, (const float2*)table, Lt, xyz_min,
                           xyz_extent, (const v8*)weights_packed, mode, sigmas, rgbs, (v8*)enc_cache, order);
    });
    NCN_LAUNCH_CHECK("ncn_field_fwd");
    return 0;
}

int ncn_field_bwd_blocks(int64_t n) { return bwd_blocks_of(n); }

int64_t ncn_field_bwd_dE_floats(int64_t n) { return n > 0 ? DeWs(n).floats() : 0; }

int ncn_field_bwd_mlp(const float* xyzs, const float* dirs, int64_t n, const int32_t* n_dev, const int32_t* order,
                      const uint16_t* weights_packed, int precision, const uint16_t* enc_cache, const float* dL_dsigmas,
                      const float* dL_drgbs, const float* loss_scale, float* slab, float* dE_ws, float* level_max,
                      void* stream) {
    if (n <= 0) return 0;
    if (const int e = bwd_mlp_check("ncn_field_bwd_mlp", precision, nullptr, dE_ws, enc_cache, weights_packed, nullptr,
                                    false, level_max, xyzs_unaligned(xyzs)))
        return e;
    launch_bwd_part<BWD_ALL>(precision, ncn_field_bwd_blocks(n), (hipStream_t)stream, xyzs, dirs, n, n_dev,
                             weights_packed, enc_cache, dL_dsigmas, dL_drgbs, loss_scale, dE_ws, slab, level_max, order,
                             nullptr, nullptr);
    NCN_LAUNCH_CHECK("ncn_field_bwd_mlp");
    return 0;
}

int ncn_field_bwd_mlp_din(const float* xyzs, const float* dirs, int64_t n, const int32_t* n_dev, const int32_t* order,
                          const uint16_t* weights_packed, int precision, const uint16_t* enc_cache,
                          const float* dL_dsigmas, const float* dL_drgbs, const float* loss_scale, float* slab,
                          float* dE_ws, float* level_max, const float* w_master, float* dL_ddirs, void* stream) {
    if (n <= 0) return 0;
    const char* own = !dirs ? "no direction gradient without dirs (density mode)"
                            : !(w_master && dL_ddirs) ? "w_master and dL_ddirs required" : nullptr;
    if (const int e = bwd_mlp_check("ncn_field_bwd_mlp_din", precision, own, dE_ws, enc_cache, weights_packed, nullptr,
                                    false, level_max, xyzs_unaligned(xyzs)))
        return e;
    launch_bwd_part<BWD_ALL, true>(precision, ncn_field_bwd_blocks(n), (hipStream_t)stream, xyzs, dirs, n, n_dev,
                                   weights_packed, enc_cache, dL_dsigmas, dL_drgbs, loss_scale, dE_ws, slab, level_max,
                                   order, nullptr, nullptr, w_master, dL_ddirs);
    NCN_LAUNCH_CHECK("ncn_field_bwd_mlp_din");
    return 0;
}

int ncn_field_bwd_dx(const float* xyzs, int64_t n, const int32_t* n_dev, const int32_t* order, const float* table,
                     const uint32_t* levels, float xyz_min, float xyz_extent, const float* dE_ws, float* dL_dxyzs,
                     void* stream) {
    if (n <= 0) return 0;
    NCN_REQUIRE(xyzs && table && levels && dE_ws && dL_dxyzs, hipErrorInvalidValue,
                "ncn_field_bwd_dx: xyzs, table, levels, dE_ws and dL_dxyzs required");
    NCN_REQUIRE(xyz_extent > 0.f, hipErrorInvalidValue, "ncn_field_bwd_dx: xyz_extent must be positive");
    NCN_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)dE_ws & 15) == 0, hipErrorInvalidValue,
                "ncn_field_bwd_dx: table 8-byte, dE_ws 16-byte aligned");
    const LevelTable Lt = make_table(levels);
    hipLaunchKernelGGL(field_bwd_dx_kernel, dim3(fwd_grid(n)), dim3(256), 0, (hipStream_t)stream, xyzs, n, n_dev, order,
                       (const float2*)table, Lt, xyz_min, xyz_extent, dE_ws, dL_dxyzs);
    NCN_LAUNCH_CHECK("ncn_field_bwd_dx");
    return 0;
}

// per 16-sample group: 64 lanes x 4 operand values (2 B) + 16 fp32 row-0 elements = 144 floats
int64_t ncn_field_bwd_stash_floats(int64_t n) { return n > 0 ? 144 * ((n + 15) / 16) : 0; }

// the sigma pass fits two workgroups per CU (compact LDS): twice the one-pass grid, at most 512
int ncn_field_bwd_part_blocks(int64_t n, int part) {
    const int nb = ncn_field_bwd_blocks(n);
    return part == 2 ? std::min(512, 2 * nb) : nb;
}

int ncn_field_bwd_mlp_part(const float* xyzs, const float* dirs, int64_t n, const int32_t* n_dev, const int32_t* order,
                           const uint16_t* weights_packed, int precision, const uint16_t* enc_cache,
                           const float* dL_dsigmas, const float* dL_dsigmas2, const float* dL_drgbs,
                           const float* loss_scale, int part, int n_blocks, float* slab, float* dE_ws,
                           float* level_max, float* dh_stash, void* stream) {
    if (n <= 0) return 0;
    if (const int e = bwd_mlp_check("ncn_field_bwd_mlp_part", precision,
                                    part == 1 || part == 2 || part == 3 ? nullptr : "part must be 1 (rgb), 2 (sigma) or 3 (both)",
                                    dE_ws, enc_cache, weights_packed, dh_stash, true, level_max,
                                    part == 3 || dh_stash ? nullptr : "dh_stash required for a split pass"))
        return e;
    const int cap = ncn_field_bwd_part_blocks(n, part), nb = n_blocks > 0 ? std::min(n_blocks, cap) : cap;
    const auto launch = part == 1 ? launch_bwd_part<BWD_RGB> : part == 2 ? launch_bwd_part<BWD_SIGMA> : launch_bwd_part<BWD_ALL>;
    launch(precision, nb, (hipStream_t)stream, xyzs, dirs, n, n_dev, weights_packed, enc_cache, dL_dsigmas, dL_drgbs,
           loss_scale, dE_ws, slab, level_max, order, dL_dsigmas2, dh_stash, nullptr, nullptr);
    NCN_LAUNCH_CHECK("ncn_field_bwd_mlp_part");
    return 0;
}

int ncn_field_scatter_wgrad(const float* xyzs, int64_t n, const int32_t* n_dev, const int32_t* order,
                            const uint32_t* levels, float xyz_min, float xyz_extent, const float* dE_ws,
                            const float* level_max, int level_lo, int level_hi, int max_blocks, float* grad_table,
                            const float* slab, int n_blocks_sigma, int n_blocks_rgb, float* grad_w, void* stream) {
    if (n <= 0 || level_hi <= level_lo)
        return slab ? ncn_field_reduce_wgrad_parts(slab, n_blocks_sigma, n_blocks_rgb, grad_w, stream) : 0;
    NCN_REQUIRE(0 <= level_lo && level_hi <= 16, hipErrorInvalidValue, "ncn_field_scatter: levels must lie in [0, 16)");
    NCN_REQUIRE(((uintptr_t)dE_ws & 15) == 0 && ((uintptr_t)xyzs & 15) == 0, hipErrorInvalidValue,
                "ncn_field_scatter: dE_ws and xyzs must be 16-byte aligned");
    NCN_REQUIRE(!slab || grad_w, hipErrorInvalidValue, "ncn_field_scatter_wgrad: grad_w required with a slab");
    const LevelTable Lt = make_table(levels);
    int grid = scatter_grid(n);
    if (max_blocks > 0) grid = std::min(grid, max_blocks * (1024 / SC_THREADS));  // (max_blocks: CUs)
    hipLaunchKernelGGL(field_scatter_kernel, dim3(grid), dim3(SC_THREADS), 0, (hipStream_t)stream, xyzs, n, n_dev, Lt,
                       xyz_min, xyz_extent, dE_ws, grad_table, level_max, ncn_field_bwd_blocks(n),
                       level_lo, level_hi, order, slab, n_blocks_sigma, n_blocks_rgb, grad_w,
                       (unsigned*)const_cast<float*>(dE_ws + DeWs(n).queue()) + 2 * level_lo);
    NCN_LAUNCH_CHECK("ncn_field_scatter");
    return 0;
}

int ncn_field_scatter_positions(const float* xyzs, int64_t n, const int32_t* n_dev, float* dE_ws, void* stream) {
    if (n <= 0) return 0;
    NCN_REQUIRE(((uintptr_t)dE_ws & 15) == 0 && ((uintptr_t)xyzs & 15) == 0, hipErrorInvalidValue,
                "ncn_field_scatter_positions: dE_ws and xyzs must be 16-byte aligned");
    const int pgrid = (int)std::max<int64_t>(1, std::min<int64_t>(1024, cdiv(cdiv(n, 4), 256)));
    const int all = (1 << SC_N_CLASSES) - 1;
    hipLaunchKernelGGL(sc_perm_positions_kernel, dim3(pgrid), dim3(256), 0, (hipStream_t)stream, xyzs, n, n_dev, all,
                       dE_ws + DeWs(n).positions(), dE_ws + DeWs::POS_MASK, (float)all);
    NCN_LAUNCH_CHECK("ncn_field_scatter_positions");
    return 0;
}

int ncn_field_scatter(const float* xyzs, int64_t n, const int32_t* n_dev, const int32_t* order, const uint32_t* levels,
                      float xyz_min, float xyz_extent, const float* dE_ws, const float* level_max, int level_lo,
                      int level_hi, int max_blocks, float* grad_table, void* stream) {
    return ncn_field_scatter_wgrad(xyzs, n, n_dev, order, levels, xyz_min, xyz_extent, dE_ws, level_max, level_lo,
                                   level_hi, max_blocks, grad_table, nullptr, 0, 0, nullptr, stream);
}

int ncn_field_bwd(const float* xyzs, const float* dirs, int64_t n, const int32_t* n_dev, const int32_t* order,
                  const uint32_t* levels, float xyz_min, float xyz_extent, const uint16_t* weights_packed, int precision,
                  const uint16_t* enc_cache, const float* dL_dsigmas, const float* dL_drgbs, const float* loss_scale,
                  float* grad_table, float* slab, float* dE_ws, float* level_max, void* stream) {
    if (const int e = ncn_field_bwd_mlp(xyzs, dirs, n, n_dev, order, weights_packed, precision, enc_cache, dL_dsigmas,
                                        dL_drgbs, loss_scale, slab, dE_ws, level_max, stream))
        return e;
    return ncn_field_scatter(xyzs, n, n_dev, order, levels, xyz_min, xyz_extent, dE_ws, level_max, 0, 16, 0,
                             grad_table, stream);
}

int ncn_field_reduce_wgrad(const float* slab, int n_blocks, float* grad_w, void* stream) {
    return reduce_wgrad("ncn_field_reduce_wgrad", slab, n_blocks, n_blocks, grad_w, stream);
}

int ncn_field_reduce_wgrad_parts(const float* slab, int n_blocks_sigma, int n_blocks_rgb, float* grad_w,
                                 void* stream) {
    return reduce_wgrad("ncn_field_reduce_wgrad_parts", slab, n_blocks_sigma, n_blocks_rgb, grad_w, stream);
}
}  // extern "C"
