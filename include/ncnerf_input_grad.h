/*
 * ncnerf_input_grad.h — the field's input gradients in the split backward: the direction gradient
 * out of the rgb part of ncn_field_bwd_mlp_part (ncnerf.h), for a backward that runs in parts — a
 * model with the semantic / normal heads (ncnerf_heads.h) under camera pose refinement, where each
 * head adds its dL/dh into the stash between the two parts.  A seventh header beside ncnerf.h,
 * ncnerf_metrics.h, ncnerf_geom.h, ncnerf_mesh.h, ncnerf_heads.h and ncnerf_sem.h, in the same
 * grammar and under the same rules (ncnerf.h, top): plain device pointers, `void* stream` last,
 * nothing allocated, nothing synchronised, 0 or a hipError_t returned.  THIS FILE IS PARSED by
 * ncnerf_amd/_lib.py exactly as ncnerf.h is, into a table of its own; every entry point here returns
 * int.  (The kernel is field_bwd_kernel<T, BWD_RGB, true> of csrc/field_bwd_mlp.h, instantiated in
 * csrc/field_rgb_din.hip, which defines the entry point.)
 */
#ifndef NCNERF_INPUT_GRAD_H
#define NCNERF_INPUT_GRAD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- part 1 (rgb) of ncn_field_bwd_mlp_part that also writes dL_ddirs, (n, 3) fp32 in SAMPLE order
 *      whatever `order` is.  Every other argument is part 1's: dL_drgbs may be NULL (zeros), n_blocks
 *      > 0 caps the grid at ncn_field_bwd_part_blocks(n, 1), w_master is the NCN_FIELD_NW fp32
 *      masters (W3's direction columns are read from it, as ncn_field_bwd_mlp_din reads them).
 *      - slab (the tiles of W3..W5), dh_stash and level_max are bit for bit part 1's on the same grid;
 *        dE_ws receives what part 1 writes into it (the positions of the two coarse unit classes).
 *      - dL_ddirs is bit for bit ncn_field_bwd_mlp_din's for the same dL_drgbs: W3[:, 0:3]^T dD3 in
 *        fp32, rounded to the operand type at the chain's scale S, divided by S, then the
 *        normalisation's backward in fp32.  The heads read h, never d: their gradient cannot enter it,
 *        so it is complete when this part ends.  Rows [*n_dev, n) are written as zeros.
 *      - dirs NULL, or w_master / dL_ddirs NULL, is hipErrorInvalidValue (NCN_REQUIRE) with nothing
 *        launched; so is a precision other than NCN_PREC_F16 / NCN_PREC_BF16, a missing slab, dh_stash
 *        or level_max, and a misaligned dE_ws / enc_cache / weights_packed / dh_stash (16 bytes).
 *      - No atomics: two runs are bit-identical.
 *      - ORDERING towards part 2 (ncn_field_bwd_mlp_part, part = 2): as part 1's — part 2 reads the
 *        stash and max-reduces into the level_max rows zeroed here, so it is stream-ordered after
 *        this launch has COMPLETED on the same stash and level_max.  dL/dx of the same backward is
 *        ncn_field_bwd_dx on the dE workspace once part 2 has run. ---- */
int ncn_field_bwd_mlp_rgb_din(const float* xyzs, const float* dirs, int64_t n, const int32_t* n_dev, const int32_t* order,
                              const uint16_t* weights_packed, int precision, const uint16_t* enc_cache,
                              const float* dL_drgbs, const float* loss_scale, int n_blocks, float* slab, float* dE_ws,
                              float* level_max, float* dh_stash, const float* w_master, float* dL_ddirs, void* stream);

#ifdef __cplusplus
}
#endif
#endif
