#pragma once
// Host side of the MLP-backward entry points, shared by the translation units that instantiate
// field_bwd_kernel (field.hip; field_rgb_din.hip): the operand ladder, the entries' common argument
// checks and the launch of one part.
#include "field_bwd_mlp.h"
namespace ncn {
// The fp16 / bf16 ladder: f gets a tag whose ::type is the operand type of `precision` (checked by the caller).
template <typename T> struct Operand { typedef T type; };
template <typename F>
static void with_operand(int precision, F&& f) {
    if (precision == NCN_PREC_F16) f(Operand<_Float16>{});
    else f(Operand<__bf16>{});
}

// The argument checks of the MLP-backward entries in their common order: the precision, the
// entry's own requirements (`own`: the message of the first one violated, or null), the alignment
// (`part_entry`: with dh_stash), level_max, and the entry's last requirement (`last`, as `own`).
static int bwd_mlp_check(const char* name, int precision, const char* own, const void* dE_ws, const void* enc,
                         const void* wp, const void* stash, bool part_entry, const void* level_max, const char* last) {
    NCN_REQUIRE(precision == NCN_PREC_F16 || precision == NCN_PREC_BF16, hipErrorInvalidValue,
                "%s: precision must be NCN_PREC_F16 or NCN_PREC_BF16", name);
    NCN_REQUIRE(!own, hipErrorInvalidValue, "%s: %s", name, own);
    NCN_REQUIRE((((uintptr_t)dE_ws | (uintptr_t)enc | (uintptr_t)wp | (uintptr_t)stash) & 15) == 0, hipErrorInvalidValue,
                "%s: dE_ws / enc_cache / weights_packed%s must be 16-byte aligned", name, part_entry ? " / dh_stash" : "");
    NCN_REQUIRE(level_max != nullptr, hipErrorInvalidValue, "%s: level_max workspace required", name);
    NCN_REQUIRE(!last, hipErrorInvalidValue, "%s: %s", name, last);
    return 0;
}

template <int PART, bool DIN = false>
static void launch_bwd_part(int precision, int nb, hipStream_t st, const float* xyzs, const float* dirs, int64_t n,
                            const int32_t* n_dev, const uint16_t* wp, const uint16_t* enc, const float* dsig,
                            const float* drgb, const float* loss_scale, float* dE_ws, float* slab, float* level_max,
                            const int32_t* order, const float* dsig2, float* stash, const float* w_master = nullptr,
                            float* dL_ddirs = nullptr) {
    with_operand(precision, [&](auto op) {
        typedef typename decltype(op)::type T;
        hipLaunchKernelGGL((field_bwd_kernel<T, PART, DIN>), dim3(nb), dim3(BWD_THREADS), 0, st, dirs, n, n_dev, wp,
                           (const typename Mfma<T>::v8*)enc, dsig, drgb, loss_scale, dE_ws, slab, level_max, order, dsig2,
                           stash, xyzs, w_master, dL_ddirs);
    });
}
}  // namespace ncn
