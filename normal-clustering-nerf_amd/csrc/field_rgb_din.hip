// The rgb part of the field's split MLP backward with the direction gradient out
// (ncn_field_bwd_mlp_rgb_din, include/ncnerf_input_grad.h): field_bwd_kernel<T, BWD_RGB, true> of
// field_bwd_mlp.h, the launch a model with heads makes under pose refinement.
// A translation unit of its own, beside field.hip, on purpose: instantiated in field.hip next to the
// plain rgb part, it changes the code the compiler emits for that kernel (the offsets of its
// transposed LDS reads are no longer folded into the instructions: 21 more vector adds per step),
// and no existing kernel may change with this one.  Here field.hip's kernels are what they were.
// The floating-point contraction is the compiler's default, as in field.hip: dL_ddirs is bit for
// bit the one-pass form's (ncn_field_bwd_mlp_din).
#include <algorithm>
#include "../../include/ncnerf_input_grad.h"
#include "field_bwd_launch.h"

using namespace ncn;

extern "C" {
int ncn_field_bwd_mlp_rgb_din(const float* xyzs, const float* dirs, int64_t n, const int32_t* n_dev, const int32_t* order,
                              const uint16_t* weights_packed, int precision, const uint16_t* enc_cache,
                              const float* dL_drgbs, const float* loss_scale, int n_blocks, float* slab, float* dE_ws,
                              float* level_max, float* dh_stash, const float* w_master, float* dL_ddirs, void* stream) {
    if (n <= 0) return 0;
    const char* own = !dirs ? "no direction gradient without dirs"
                            : !(w_master && dL_ddirs) ? "w_master and dL_ddirs required" : nullptr;
    if (const int e = bwd_mlp_check("ncn_field_bwd_mlp_rgb_din", precision, own, dE_ws, enc_cache, weights_packed, dh_stash,
                                    true, level_max, slab && dh_stash ? nullptr : "slab and dh_stash required"))
        return e;
    const int cap = ncn_field_bwd_part_blocks(n, 1), nb = n_blocks > 0 ? std::min(n_blocks, cap) : cap;
    launch_bwd_part<BWD_RGB, true>(precision, nb, (hipStream_t)stream, xyzs, dirs, n, n_dev, weights_packed, enc_cache,
                                   nullptr, dL_drgbs, loss_scale, dE_ws, slab, level_max, order, nullptr, dh_stash,
                                   w_master, dL_ddirs);
    NCN_LAUNCH_CHECK("ncn_field_bwd_mlp_rgb_din");
    return 0;
}
}
