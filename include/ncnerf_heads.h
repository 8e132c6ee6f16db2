/*
 * ncnerf_heads.h — the semantic and normal heads of NGPMT (models/ngp_mt.py:116-140, 222-227: sem_net
 * and norm_net on the 16 sigma_net features h) and the compositing of their channels.  A fifth header
 * beside ncnerf.h, ncnerf_metrics.h, ncnerf_geom.h and ncnerf_mesh.h, in the same grammar and under the
 * same rules (ncnerf.h, top): plain device pointers, `void* stream` last, nothing allocated, nothing
 * synchronised, 0 or a hipError_t returned.  THIS FILE IS PARSED by ncnerf_amd/_lib.py exactly as
 * ncnerf.h is, into a table of its own; every entry point returns int.
 *
 * HEAD NETWORK.  tcnn FullyFusedMLP(16 -> 64 -> 64 -> n_out): ReLU, no output activation, no biases.
 *   1 <= n_out <= NCN_HEAD_MAX_OUT; tcnn pads the output to a multiple of 16 rows, so with
 *   T = ceil(n_out / 16) the fp32 masters are, concatenated and row-major (out, in):
 *       Wa (64, 16) | Wb (64, 64) | Wc (16 T, 64)           NCN_HEAD_NW(n_out) floats
 *   Rows >= n_out of Wc are parameters whose outputs are discarded: their gradient is exactly 0.
 *   Operands (weights, h, the two hidden activations, the upstream gradient and the two pre-ReLU
 *   gradients) are rounded to `precision` (NCN_PREC_F16 / NCN_PREC_BF16 of ncnerf.h) at each layer
 *   input, as the field rounds its own; accumulation is fp32.
 *   h is not stored by the field: both kernels recompute it from the field's encoding cache
 *   (enc_cache of ncn_field_fwd, in its identity processing order: `order` must have been NULL) with
 *   the field's packed W1 / W2 (field_weights_packed = weights_packed of ncn_field_fwd) — the very
 *   instructions the field ran, so the same h bit for bit.
 *   n is the capacity, n_dev NULL or the device count as in ncn_field_fwd.
 * Any n_out outside [1, NCN_HEAD_MAX_OUT], or a precision that is neither, is hipErrorInvalidValue.
 */
#ifndef NCNERF_HEADS_H
#define NCNERF_HEADS_H
#include <stdint.h>

#define NCN_HEAD_MAX_OUT 48
#define NCN_HEAD_NW(n_out) (64 * 16 + 64 * 64 + 64 * 16 * (((n_out) + 15) / 16))
/* the packed fragments of one head (forward and transposed backward), whatever n_out is */
#define NCN_HEAD_PACKED_HALVES 16384
/* most channels of ncn_composite_extra_*: 3 normal channels + NCN_HEAD_MAX_OUT classes */
#define NCN_EXTRA_MAX_CH 51

#ifdef __cplusplus
extern "C" {
#endif

/* ---- packing: NCN_HEAD_PACKED_HALVES 16-bit MFMA fragments (16-byte aligned) from the
 *      NCN_HEAD_NW(n_out) fp32 masters; output tiles past T are packed as zeros.
 *      ncn_head_packed_halves returns NCN_HEAD_PACKED_HALVES, or -1 for an n_out out of range. ---- */
int ncn_head_packed_halves(int n_out);
int ncn_head_pack_weights(const float* w_master, int n_out, uint16_t* packed, int precision, void* stream);

/* ---- forward: out (n, n_out) fp32 = the unrounded accumulators of the last layer.  Rows >= *n_dev
 *      are not written. ---- */
int ncn_head_fwd(const uint16_t* enc_cache, int64_t n, const int32_t* n_dev, const uint16_t* field_weights_packed,
                 const uint16_t* head_packed, int n_out, int precision, float* out, void* stream);

/* ---- the features alone (NGPMT.density(x, return_feat=True), ngp_mt.py:157-171): h (n, 16) fp32
 *      (16-byte aligned), the unrounded accumulators of sigma_net's last layer, recomputed from the
 *      encoding cache as above.  Rows >= *n_dev are not written. ---- */
int ncn_head_feat(const uint16_t* enc_cache, int64_t n, const int32_t* n_dev, const uint16_t* field_weights_packed,
                  int precision, float* h, void* stream);

/* ---- backward, between parts 1 and 2 of ncn_field_bwd_mlp_part (stream-ordered after a completed
 *      part 1 on the same dh_stash, before part 2).  dL_dout (n, n_out) is taken times the chain's
 *      scale S (loss_scale as in ncn_field_bwd: S = *loss_scale x 128 for fp16, 1 for bf16 or NULL).
 *      Writes one weight-gradient slab row of NCN_HEAD_NW(n_out) floats per workgroup (fp32 MFMA
 *      products divided by S; ncn_head_bwd_blocks(n) rows, every element of every row written), and
 *      ADDS its dL/dh into dh_stash in the layout part 1 leaves: per 16-sample group the 64 operand
 *      tiles' values become round(float(stashed) + dL/dh) (one rounding, at the scale S) and the
 *      group's 16 fp32 row-0 values += dL/dh row 0 (fp32).  Groups past *n_dev are left alone.
 *      No float atomics: two runs give the same bits.  ncn_head_reduce_wgrad sums the slab rows in a
 *      fixed order (16 runs of consecutive rows, then the runs in order) and adds the sum to grad_w
 *      (+=). ---- */
int ncn_head_bwd_blocks(int64_t n);
int ncn_head_bwd(const uint16_t* enc_cache, int64_t n, const int32_t* n_dev, const uint16_t* field_weights_packed,
                 const uint16_t* head_packed, int n_out, int precision, const float* dL_dout, const float* loss_scale,
                 float* slab, float* dh_stash, void* stream);
int ncn_head_reduce_wgrad(const float* slab, int n_blocks, int n_w, float* grad_w, void* stream);

/* ---- compositing of extra channels through the compositor's weights.  Compositing is linear per
 *      channel with weights that depend on sigma and delta alone: rend[r][c] = sum over the samples s
 *      of ray r of ws[s] raws[s][c], ws (S) the weights ncn_composite_train_fw returns (zero behind
 *      the terminating sample), raws (S, n_ch), rays_a (n_rays, 3) int64 {ray, start, count}.
 *      fw: rend (R, n_ch) row rays_a[i][0] of every listed ray is written (zeros for a ray without
 *      samples); a wave per ray, fixed summation order.  bw: dL_draws[s][c] = dL_drend[r][c] ws[s] and
 *      dL_dws[s] = sum_c dL_drend[r][c] raws[s][c] (a fixed order) for the samples of the listed rays.
 *      Rows of ws / raws outside every ray's range are never read, and the matching rows of dL_dws /
 *      dL_draws are never written: the caller zeroes both outputs.  n_samples is the row count S of
 *      ws / raws: a range is cut to [0, S), and a row whose ray index lies outside [0, n_rays) is
 *      skipped.  1 <= n_ch <= NCN_EXTRA_MAX_CH. ---- */
int ncn_composite_extra_fw(const float* ws, const float* raws, const int64_t* rays_a, int64_t n_rays, int64_t n_samples,
                           int n_ch, float* rend, void* stream);
int ncn_composite_extra_bw(const float* dL_drend, const float* ws, const float* raws, const int64_t* rays_a,
                           int64_t n_rays, int64_t n_samples, int n_ch, float* dL_dws, float* dL_draws, void* stream);

#ifdef __cplusplus
}
#endif
#endif
