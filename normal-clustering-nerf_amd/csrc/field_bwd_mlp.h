#pragma once
#include "field_de_ws.h"
#include "field_diag.h"
#include "field_mlp.h"
namespace ncn {
// Backward, MLP pass.  A workgroup of 8 waves (one per CU: 2 waves per SIMD) takes 8 groups of 16
// samples per step.  Phase 1, every wave on its own group (inputs prefetched one step ahead):
// recompute the MLP forward from the cached encoding, back-propagate through the five layers
// (transposed products with the W^T fragments from LDS), write the encoding gradient level-major
// for the scatter pass, and put the 30 operand tiles of the weight gradient (dY and X tiles of
// every layer, transposed so that the samples are on K) into an LDS exchange area.  Phase 2,
// after a barrier: wave w owns 5 of the 40 dW tiles and accumulates them over the step's groups
// straight from the exchange area, two groups (32 samples) per K=32 MFMA.  So no wave holds all
// of dW, the two waves of a SIMD overlap their MFMA chains, and every tile is written once per
// workgroup into its slab row at the end.
constexpr int BWD_WAVES = 8;
constexpr int BWD_THREADS = 64 * BWD_WAVES;
// exchange tiles per group: dW operands, A = dY^T, B = X^T (16 features x 16 samples)
constexpr int XA5 = 0, XB5 = 1, XA4 = 5, XB4 = 9, XA3 = 13, XB3D = 17, XB3H = 18, XA2 = 19, XB2 = 20, XA1 = 24,
              XB1 = 28, N_XFRAG = 30;

// dW operands through LDS images: a C-layout tile (lane (g,r) holds [feature 4g+i][sample r]) is
// stored as a [sample][feature] image (16 rows of 32 B; lane (g,r) writes 8 B at row r, chunk g,
// chunks XOR-swizzled by row>>2 against write bank conflicts) and read back with the gfx950
// transposed read ds_read_b64_tr_b16: lane 4q+p of group g addresses row 4g+q, chunk p, and lane
// (g,i) receives column i of rows 4g..4g+3, i.e. [feature i][samples 4g..4g+3] — half of the A/B
// fragment of a product that sums over samples (the two halves of a K=32 fragment are the images
// of two groups).  (EXEC must be all ones at the read.)
template <typename V>
__device__ __forceinline__ void x_put(uint16_t* tile, int lane, V v) {
    const int g = lane >> 4, r = lane & 15;
    *(V*)(tile + r * 16 + 4 * (g ^ (r >> 2))) = v;
}
template <typename V>
__device__ __forceinline__ V x_get(const uint16_t* tile, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const short4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) short4_t*)(tile + (4 * g + q) * 16 + 4 * (p ^ g)));
    return __builtin_bit_cast(V, v);
}

// Per-group inputs of the backward (prefetched one step ahead).
// Backward parts (the split MLP pass of the training step, ncn_field_bwd_mlp_part): BWD_RGB = the
// rgb_net path alone (needs only dL/drgb: it can run while the clustering still computes the depth
// gradient) — dW3..dW5 and the rgb part of dL/dh, stashed; BWD_SIGMA = the rest: dL/dh = stash +
// TruncExp'(h0) dL/dsigma, then sigma_net and the encoding gradient, dW1, dW2.  BWD_ALL = both.
enum { BWD_RGB = 1, BWD_SIGMA = 2, BWD_ALL = 3 };
template <typename T>
struct BwdIn {
    typename Mfma<T>::v8 e;
    float dx, dy, dz, dsig, dr0, dr1, dr2;
    float px, py, pz;  // (rgb / one pass, with positions out) the sample's position
    typename Mfma<T>::v4 dq;  // (BWD_SIGMA) the stashed rgb part of dL/dh of this lane's tile, as operands
    float h0;                 // (BWD_SIGMA, g = 0) its row-0 element in fp32 (TruncExp's term is added to it)
};
template <typename T, int PART>
__device__ __forceinline__ void bwd_load(BwdIn<T>& in, int64_t grp, int64_t n, int lane,
                                         const typename Mfma<T>::v8* __restrict__ enc, const float* __restrict__ dirs,
                                         const float* __restrict__ dL_dsig, const float* __restrict__ dL_dsig2,
                                         const float* __restrict__ dL_drgb,
                                         const typename Mfma<T>::v4* __restrict__ stq, const float* __restrict__ sth0,
                                         const int32_t* __restrict__ order, float S, const float* __restrict__ xyzs) {
    const int64_t pos = grp * 16 + (lane & 15);  // processing position (enc_cache / dE order)
    const bool valid = pos < n;
    in.e = enc[grp * 64 + lane];
    in.dx = in.dy = in.dz = in.dsig = in.dr0 = in.dr1 = in.dr2 = 0.f;
    in.px = in.py = in.pz = 0.f;
    if constexpr ((PART & DE_POS_PART) != 0) {
        if (xyzs && valid) { in.px = xyzs[3 * pos]; in.py = xyzs[3 * pos + 1]; in.pz = xyzs[3 * pos + 2]; }
    }
    if constexpr (PART == BWD_SIGMA) {
        in.dq = stq[grp * 64 + lane];
        in.h0 = (lane >> 4) == 0 ? sth0[grp * 16 + (lane & 15)] : 0.f;
    }
    if (valid) {
        const int64_t s = order ? (int64_t)order[pos] : pos;
        if constexpr ((PART & BWD_RGB) != 0) {
            in.dx = dirs[3 * s]; in.dy = dirs[3 * s + 1]; in.dz = dirs[3 * s + 2];
            if (dL_drgb) { in.dr0 = dL_drgb[3 * s] * S; in.dr1 = dL_drgb[3 * s + 1] * S; in.dr2 = dL_drgb[3 * s + 2] * S; }
        }
        if constexpr ((PART & BWD_SIGMA) != 0) {
            const float ds = (dL_dsig ? dL_dsig[s] : 0.f) + (dL_dsig2 ? dL_dsig2[s] : 0.f);
            in.dsig = ds * S;
        }
    }
}

// Phase 1 for one group: forward recompute, backward through the layers, dE out, dW operands out.
__device__ __forceinline__ float lmax_upd(float m, float a, float b) {  // non-finite -> INF
    return (isfinite(a) && isfinite(b)) ? fmaxf(m, fmaxf(fabsf(a), fabsf(b))) : INFINITY;
}
// exchange tiles a pass keeps per group: the sigma pass only XA2..XB1+1 (compact layout, origin XA2)
template <int PART> constexpr int x_count() { return PART == BWD_SIGMA ? N_XFRAG - XA2 : N_XFRAG; }
template <int PART> constexpr int x_origin() { return PART == BWD_SIGMA ? XA2 : 0; }

// (DIN: the one-pass form, or the split backward's rgb part) the direction gradient's operands:
// W3's three direction columns rounded to T in LDS ([k][64 rows]), the processing order and the
// output (n, 3) in sample order
template <typename T>
struct DinCtx {
    const T* w3d;
    const int32_t* order;
    float* out;
};
template <typename T, int PART, bool DIN = false, typename FR>
__device__ __forceinline__ void bwd_group(const FR& F, uint16_t* Xw, const BwdIn<T>& cur, int64_t grp,
                                          int64_t n, int64_t n_stride, int lane, float* __restrict__ dE_out,
                                          float (&lm)[4], float inv_S, typename Mfma<T>::v4* __restrict__ stq,
                                          float* __restrict__ sth0, const DinCtx<T>* din = nullptr) {
    typedef Mfma<T> M;
    typedef typename M::v4 v4;
    typedef typename M::v8 v8;
    const int g = lane >> 4, r = lane & 15;
    const int64_t s = grp * 16 + r;
    const bool valid = s < n;
    FwdState<T> st;
    mlp_sigma<T>(F, lane, cur.e, st);
    float4_t dh;
    if constexpr ((PART & BWD_RGB) != 0) {
    float dx = cur.dx, dy = cur.dy, dz = cur.dz;
    if (valid) {
        const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
        dx /= nrm; dy /= nrm; dz /= nrm;
    }
    mlp_rgb<T>(F, lane, dx, dy, dz, st);
    // dY5: d(pre-sigmoid) = drgb * s(1-s), rows 0..2 on g==0 (the padded output rows get zero)
    float4_t dy5 = zero4();
    if (g == 0) {
        const float s0 = sigmoidf_(st.out[0]), s1 = sigmoidf_(st.out[1]), s2 = sigmoidf_(st.out[2]);
        dy5[0] = cur.dr0 * s0 * (1.f - s0);
        dy5[1] = cur.dr1 * s1 * (1.f - s1);
        dy5[2] = cur.dr2 * s2 * (1.f - s2);
    }
    const v4 dy5h = cvt4<T>(dy5);
    x_put(Xw + XA5 * 256, lane, dy5h);
#pragma unroll
    for (int b = 0; b < 4; b++) x_put(Xw + (XB5 + b) * 256, lane, st.x5[b]);
    // L5 backward -> dG2, ReLU(x5) mask -> dD4
    v4 dD4[4];
#pragma unroll
    for (int t = 0; t < 4; t++) dD4[t] = relu_mask4<T>(M::k16(F.a16(B_L5 + t, lane), dy5h, zero4()), st.x5[t]);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        x_put(Xw + (XA4 + t) * 256, lane, dD4[t]);
        x_put(Xw + (XB4 + t) * 256, lane, st.x4[t]);
    }
    // L4 backward -> dG1, ReLU(x4) mask -> dD3
    const v8 d4a = cat8<v8>(dD4[0], dD4[1]), d4b = cat8<v8>(dD4[2], dD4[3]);
    v4 dD3[4];
#pragma unroll
    for (int t = 0; t < 4; t++)
        dD3[t] = relu_mask4<T>(M::k32(F.a32(B_L4 + 2 * t + 1, lane), d4b, M::k32(F.a32(B_L4 + 2 * t, lane), d4a, zero4())),
                                st.x4[t]);
#pragma unroll
    for (int t = 0; t < 4; t++) x_put(Xw + (XA3 + t) * 256, lane, dD3[t]);
    x_put(Xw + XB3D * 256, lane, st.x3d);
    x_put(Xw + XB3H * 256, lane, st.x3h);
    if constexpr (DIN) {
        // dL/d(d/|d|) = W3[:, 0:3]^T dD3: the lane's 16 rows (tile t rows 4g..4g+3) against the
        // rounded columns in fp32, then the four row groups summed by two fixed exchanges (every
        // lane forms the same sum).  Handed on in the operand type at the chain's scale, as tcnn
        // hands a network's input gradient on, then unscaled; the normalisation's backward in fp32.
        float gi[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const v4 w = *(const v4*)(din->w3d + k * 64 + 16 * t + 4 * g);
#pragma unroll
                for (int i = 0; i < 4; i++) gi[k] = fmaf((float)w[i], (float)dD3[t][i], gi[k]);
            }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            gi[k] += __shfl_xor(gi[k], 16);
            gi[k] += __shfl_xor(gi[k], 32);
        }
        if (g == 0 && valid) {
#pragma unroll
            for (int k = 0; k < 3; k++) gi[k] = (float)(T)gi[k] * inv_S;
            const float nrm = sqrtf(cur.dx * cur.dx + cur.dy * cur.dy + cur.dz * cur.dz);
            const float nx = cur.dx / nrm, ny = cur.dy / nrm, nz = cur.dz / nrm;
            const float ng = nx * gi[0] + ny * gi[1] + nz * gi[2];
            float* o = din->out + 3 * (din->order ? (int64_t)din->order[s] : s);
            o[0] = (gi[0] - nx * ng) / nrm;
            o[1] = (gi[1] - ny * ng) / nrm;
            o[2] = (gi[2] - nz * ng) / nrm;
        }
    }
    // L3 backward -> dh (rgb path) ; + TruncExp backward on h[0]
    dh = M::k32(F.a32(B_L3, lane), cat8<v8>(dD3[0], dD3[1]), zero4());
    dh = M::k32(F.a32(B_L3 + 1, lane), cat8<v8>(dD3[2], dD3[3]), dh);
    if constexpr (PART == BWD_RGB) {  // the sigma part follows in its own pass (BWD_SIGMA)
        // stash: the operand-rounded tile (what the sigma pass converts it to anyway) and, for the
        // row-0 element that TruncExp's term is added to first, its fp32 value: 36 B per sample
        stq[grp * 64 + lane] = cvt4<T>(dh);
        if (g == 0) sth0[grp * 16 + r] = dh[0];
        return;
    }
    }
    v4 dhh;
    const float tex = __expf(fminf(fmaxf(st.h[0], -15.f), 15.f));
    if constexpr (PART == BWD_SIGMA) {  // (the same explicit fma and rounding as below: bit-identical)
        dhh = cur.dq;
        if (g == 0) dhh[0] = (T)fmaf(cur.dsig, tex, cur.h0);
    } else {  // (the split passes' order: the whole tile rounded as the rgb pass stashes it, then the
              // row-0 element recomputed with the TruncExp term — keeps the two forms bit-identical)
        dhh = cvt4<T>(dh);
        if (g == 0) dhh[0] = (T)fmaf(cur.dsig, tex, dh[0]);
    }
    constexpr int XO = x_origin<PART>();
    x_put(Xw + (XA2 - XO) * 256, lane, dhh);
#pragma unroll
    for (int b = 0; b < 4; b++) x_put(Xw + (XB2 - XO + b) * 256, lane, st.x2[b]);
    // L2 backward -> dH1, ReLU(x2) mask -> dD1
    v4 dD1[4];
#pragma unroll
    for (int t = 0; t < 4; t++) dD1[t] = relu_mask4<T>(M::k16(F.a16(B_L2 + t, lane), dhh, zero4()), st.x2[t]);
#pragma unroll
    for (int t = 0; t < 4; t++) x_put(Xw + (XA1 - XO + t) * 256, lane, dD1[t]);
    const v4 e0 = v4{cur.e[0], cur.e[1], cur.e[2], cur.e[3]}, e1 = v4{cur.e[4], cur.e[5], cur.e[6], cur.e[7]};
    x_put(Xw + (XB1 - XO) * 256, lane, e0);
    x_put(Xw + (XB1 - XO + 1) * 256, lane, e1);
    // L1 backward -> dE (tile t holds levels 8t+2g, 8t+2g+1)
    const v8 d1a = cat8<v8>(dD1[0], dD1[1]), d1b = cat8<v8>(dD1[2], dD1[3]);
    float4_t dE[2];
#pragma unroll
    for (int t = 0; t < 2; t++)
        dE[t] = M::k32(F.a32(B_L1 + 2 * t + 1, lane), d1b, M::k32(F.a32(B_L1 + 2 * t, lane), d1a, zero4()));
    // The encoding gradient leaves in the MLP operand type, as tcnn hands its network's input gradient
    // (type T) to the grid backward: fp16 at the chain's scale S (the scatter divides by S), bf16
    // unscaled — level-major [16][n_stride] pairs behind the workspace header (dE_pairs), half the
    // bytes of f32 pairs.  fp16 overflow gives inf: the level's max is then non-finite, the scatter
    // adds it straight to the gradient and the GradScaler skips the step, as tcnn's would.
    typedef T t2 __attribute__((ext_vector_type(2)));
    const t2 q[4] = {t2{(T)dE[0][0], (T)dE[0][1]}, t2{(T)dE[0][2], (T)dE[0][3]}, t2{(T)dE[1][0], (T)dE[1][1]},
                     t2{(T)dE[1][2], (T)dE[1][3]}};
    // per-level max |dE| of this lane's levels (2g, 2g+1, 8+2g, 9+2g), of the stored values (loss
    // scale off: an exact power of two): the scatter's fixed-point scale
#pragma unroll
    for (int j = 0; j < 4; j++) lm[j] = lmax_upd(lm[j], (float)q[j][0] * inv_S, (float)q[j][1] * inv_S);
    if (valid) {
        t2* o = (t2*)dE_out;
        o[(int64_t)(2 * g) * n_stride + s] = q[0];
        o[(int64_t)(2 * g + 1) * n_stride + s] = q[1];
        o[(int64_t)(8 + 2 * g) * n_stride + s] = q[2];
        o[(int64_t)(9 + 2 * g) * n_stride + s] = q[3];
    }
}

// Phase 2: the dW tiles owned by wave `wid`, accumulated over the exchange tiles of `ng` groups,
// two groups per K=32 MFMA (an odd last group is paired with zeros).  Ownership (5 tiles each):
// waves 0-3: W4 row-block a = wid (4 tiles) + W5 column block wid; waves 4-5: W3 row-blocks
// 2(wid-4), +1 (d/pad and h tiles) + W2 block wid-4; waves 6-7: W1 row-blocks 2(wid-6), +1 (two K
// tiles) + W2 block wid-4.
template <typename T, int NX = N_XFRAG, int XO = 0>
__device__ __forceinline__ typename Mfma<T>::v8 x_pair(const uint16_t* X, int q, int ng, int tile, int lane) {
    typedef typename Mfma<T>::v4 v4;
    const v4 a = x_get<v4>(X + (q * NX + tile - XO) * 256, lane);
    const v4 b = q + 1 < ng ? x_get<v4>(X + ((q + 1) * NX + tile - XO) * 256, lane) : v4{0, 0, 0, 0};
    return cat8<typename Mfma<T>::v8>(a, b);
}
template <typename T, int PART>
__device__ __forceinline__ void bwd_dw(const uint16_t* X, int ng, int wid, int lane, float4_t (&acc)[5]) {
    typedef Mfma<T> M;
    typedef typename M::v8 v8;
    if constexpr (PART == BWD_SIGMA) {  // 12 tiles: W1 (4 row x 2 col blocks) one per wave, W2 on waves 0-3
        constexpr int NX = x_count<PART>(), XO = x_origin<PART>();
        if (ng == BWD_WAVES) {  // a full step, unrolled: its LDS reads can leave ahead of the MFMAs (same sequence)
#pragma unroll
            for (int q = 0; q < BWD_WAVES; q += 2) {
                acc[0] = M::k32(x_pair<T, NX, XO>(X, q, BWD_WAVES, XA1 + (wid >> 1), lane),
                                x_pair<T, NX, XO>(X, q, BWD_WAVES, XB1 + (wid & 1), lane), acc[0]);
                if (wid < 4)
                    acc[1] = M::k32(x_pair<T, NX, XO>(X, q, BWD_WAVES, XA2, lane),
                                    x_pair<T, NX, XO>(X, q, BWD_WAVES, XB2 + wid, lane), acc[1]);
            }
            return;
        }
        for (int q = 0; q < ng; q += 2) {
            acc[0] = M::k32(x_pair<T, NX, XO>(X, q, ng, XA1 + (wid >> 1), lane),
                            x_pair<T, NX, XO>(X, q, ng, XB1 + (wid & 1), lane), acc[0]);
            if (wid < 4)
                acc[1] = M::k32(x_pair<T, NX, XO>(X, q, ng, XA2, lane), x_pair<T, NX, XO>(X, q, ng, XB2 + wid, lane),
                                acc[1]);
        }
        return;
    }
    if constexpr (PART == BWD_RGB) {  // 28 tiles: W4 on waves 0-3 (4 each), W3 row block + W5 on waves 4-7
        for (int q = 0; q < ng; q += 2) {
            if (wid < 4) {
                const v8 A4 = x_pair<T>(X, q, ng, XA4 + wid, lane);
#pragma unroll
                for (int b = 0; b < 4; b++) acc[b] = M::k32(A4, x_pair<T>(X, q, ng, XB4 + b, lane), acc[b]);
            } else {
                const v8 A3 = x_pair<T>(X, q, ng, XA3 + wid - 4, lane);
                acc[0] = M::k32(A3, x_pair<T>(X, q, ng, XB3D, lane), acc[0]);
                acc[1] = M::k32(A3, x_pair<T>(X, q, ng, XB3H, lane), acc[1]);
                acc[4] = M::k32(x_pair<T>(X, q, ng, XA5, lane), x_pair<T>(X, q, ng, XB5 + wid - 4, lane), acc[4]);
            }
        }
        return;
    }
    for (int q = 0; q < ng; q += 2) {  // (the one-pass form: the ownership above)
        if (wid < 4) {
            const v8 A4 = x_pair<T>(X, q, ng, XA4 + wid, lane);
#pragma unroll
            for (int b = 0; b < 4; b++) acc[b] = M::k32(A4, x_pair<T>(X, q, ng, XB4 + b, lane), acc[b]);
            acc[4] = M::k32(x_pair<T>(X, q, ng, XA5, lane), x_pair<T>(X, q, ng, XB5 + wid, lane), acc[4]);
        } else if (wid < 6) {
            const v8 Bd = x_pair<T>(X, q, ng, XB3D, lane), Bh = x_pair<T>(X, q, ng, XB3H, lane);
#pragma unroll
            for (int aa = 0; aa < 2; aa++) {
                const v8 A3 = x_pair<T>(X, q, ng, XA3 + 2 * (wid - 4) + aa, lane);
                acc[2 * aa] = M::k32(A3, Bd, acc[2 * aa]);
                acc[2 * aa + 1] = M::k32(A3, Bh, acc[2 * aa + 1]);
            }
            acc[4] = M::k32(x_pair<T>(X, q, ng, XA2, lane), x_pair<T>(X, q, ng, XB2 + wid - 4, lane), acc[4]);
        } else {
            const v8 B0 = x_pair<T>(X, q, ng, XB1, lane), B1 = x_pair<T>(X, q, ng, XB1 + 1, lane);
#pragma unroll
            for (int aa = 0; aa < 2; aa++) {
                const v8 A1 = x_pair<T>(X, q, ng, XA1 + 2 * (wid - 6) + aa, lane);
                acc[2 * aa] = M::k32(A1, B0, acc[2 * aa]);
                acc[2 * aa + 1] = M::k32(A1, B1, acc[2 * aa + 1]);
            }
            acc[4] = M::k32(x_pair<T>(X, q, ng, XA2, lane), x_pair<T>(X, q, ng, XB2 + wid - 4, lane), acc[4]);
        }
    }
}

// The owned tiles (C layout: lane (g,r) = rows 4g+i, column r) into the workgroup's slab row.
// W3 columns: the h tile's column r is input 3+r; the [d, pad] tile's column q is input q (d) or
// 16+q (the 13 constant-1 padding inputs, whose gradient is the plain sum of dY).
// (A split pass stores only its own tiles: the other pass writes the rest of the same slab row.)
template <int PART>
__device__ __forceinline__ void bwd_store_dw(float* __restrict__ out, int wid, int lane, float4_t (&acc)[5], float inv_S) {
    const int g = lane >> 4, r = lane & 15;
#pragma unroll
    for (int t = 0; t < 5; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[t][i] *= inv_S;
    if constexpr (PART == BWD_SIGMA) {  // (bwd_dw's split-pass tile ownership)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int row = 4 * g + i;
            out[W1_OFF + (16 * (wid >> 1) + row) * 32 + 16 * (wid & 1) + r] = acc[0][i];
            if (wid < 4) out[W2_OFF + row * 64 + 16 * wid + r] = acc[1][i];
        }
        return;
    }
    if constexpr (PART == BWD_RGB) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int row = 4 * g + i;
            if (wid < 4) {
#pragma unroll
                for (int b = 0; b < 4; b++) out[W4_OFF + (16 * wid + row) * 64 + 16 * b + r] = acc[b][i];
            } else {
                const int orow = 16 * (wid - 4) + row;
                out[W3_OFF + orow * 32 + (r < 3 ? r : 16 + r)] = acc[0][i];
                out[W3_OFF + orow * 32 + 3 + r] = acc[1][i];
                out[W5_OFF + row * 64 + 16 * (wid - 4) + r] = acc[4][i];
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = 4 * g + i;
        if (wid < 4) {  // (the one-pass form)
#pragma unroll
            for (int b = 0; b < 4; b++) out[W4_OFF + (16 * wid + row) * 64 + 16 * b + r] = acc[b][i];
            out[W5_OFF + row * 64 + 16 * wid + r] = acc[4][i];
        } else if (wid < 6) {
#pragma unroll
            for (int aa = 0; aa < 2; aa++) {
                const int orow = 16 * (2 * (wid - 4) + aa) + row;
                out[W3_OFF + orow * 32 + (r < 3 ? r : 16 + r)] = acc[2 * aa][i];
                out[W3_OFF + orow * 32 + 3 + r] = acc[2 * aa + 1][i];
            }
            out[W2_OFF + row * 64 + 16 * (wid - 4) + r] = acc[4][i];
        } else {
#pragma unroll
            for (int aa = 0; aa < 2; aa++) {
                const int orow = 16 * (2 * (wid - 6) + aa) + row;
                out[W1_OFF + orow * 32 + r] = acc[2 * aa][i];
                out[W1_OFF + orow * 32 + 16 + r] = acc[2 * aa + 1][i];
            }
            out[W2_OFF + row * 64 + 16 * (wid - 4) + r] = acc[4][i];
        }
    }
}

// one 8-wave workgroup per CU on 256 CUs; at least ~4 steps of 8 groups each
__host__ __device__ inline int bwd_blocks_of(int64_t n) {
    const int64_t groups = (n + 15) / 16;
    const int64_t b = (groups + 31) / 32;
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

// The workgroup's LDS: the sigma pass keeps only the sigma_net fragments and its 11 exchange tiles
// per group (57 KB: two workgroups per CU); the others all 34 + 8 fragments and 30 tiles (158 KB).
template <typename T, int PART>
struct BwdLds {
    static constexpr bool SIGONLY = PART == BWD_SIGMA;
    static constexpr int NF32 = SIGONLY ? N_SIG32 : N_FRAG32, NF16 = SIGONLY ? N_SIG16 : N_FRAG16, NX = x_count<PART>();
    typename Mfma<T>::v8 F32s[NF32 * 64];
    typename Mfma<T>::v4 F16s[NF16 * 64];
    __attribute__((aligned(16))) uint16_t X[BWD_WAVES * NX * 256];  // dW operand images
};

// The pass as a device function of the workgroup's index bid in [0, nblk) and its LDS (the three
// arrays of BwdLds), so that it can also run as one role of a wider launch (split_fused.hip);
// field_bwd_kernel below is the launch of its own.  rgb_on (BWD_RGB): NULL, or a device flag whose
// zero makes the pass take dL_drgb as zeros.
template <typename T, int PART = BWD_ALL, bool DIN = false>
__device__ __forceinline__ void field_bwd_body(
    typename Mfma<T>::v8* __restrict__ const F32s, typename Mfma<T>::v4* __restrict__ const F16s,
    uint16_t* __restrict__ const X, const int bid, const int nblk, const float* __restrict__ rgb_on,
    const float* __restrict__ dirs, int64_t n, const int32_t* __restrict__ n_dev, const uint16_t* __restrict__ wpacked,
    const typename Mfma<T>::v8* __restrict__ enc_cache, const float* __restrict__ dL_dsig,
    const float* __restrict__ dL_drgb, const float* __restrict__ loss_scale, float* __restrict__ dE_out,
    float* __restrict__ slab, float* __restrict__ level_max, const int32_t* __restrict__ order,
    const float* __restrict__ dL_dsig2, float* __restrict__ stash, const float* __restrict__ xyzs,
    const float* __restrict__ w_master, float* __restrict__ dL_ddirs) {
    static_assert(!DIN || (PART & BWD_RGB) != 0, "the direction gradient leaves with the rgb_net path, not the sigma part");
    typedef typename Mfma<T>::v4 v4;
    if (rgb_on && *rgb_on == 0.f) dL_drgb = nullptr;  // (uniform; bwd_load then leaves dr0..2 at zero)
    // AMP loss scale (GradScaler of the reference's precision=16 run) times tcnn's fp16 module loss
    // scale (128): the fp16 chain sees the upstream gradients times S (a power of two), dE and dW
    // leave it divided by S.  bf16 (fp32's exponent range) runs unscaled, as tcnn's non-fp16 modules.
    const float S = loss_scale ? *loss_scale * (Mfma<T>::f16 ? NCN_TCNN_LOSS_SCALE : 1.f) : 1.f, inv_S = 1.f / S;
    typedef typename Mfma<T>::v8 v8;
    const DeWs ws(n);  // the dE workspace (field_de_ws.h): header, [16][e_stride] pairs, positions, queue
    const int64_t n_stride = ws.e_stride;
    float* const dE_pairs = dE_out ? dE_out + ws.row(0) : nullptr;
    if (PART != BWD_RGB && dE_out && bid == 0 && threadIdx.x < SC_QUEUE_WORDS) {
        if (threadIdx.x == 0) {
            dE_out[DeWs::INV_S] = inv_S;
            dE_out[DeWs::OPERAND] = Mfma<T>::f16 ? 0.f : 1.f;
        }
        ((unsigned*)(dE_out + ws.queue()))[threadIdx.x] = 0u;  // the scatter's unit queue
    }
    // (rgb / one pass) the sample positions in the scatter's per-class load order (sc_perm): lane
    // (g, r) writes sample r's position into class g's array.  In the processing order of `order`
    // the scatter gathers them itself (no positions written).
    const float* pos_src = ((PART & DE_POS_PART) != 0 && dE_out && !order) ? xyzs : nullptr;
    float* const pos_out = pos_src ? dE_out + ws.positions() : nullptr;
    const int64_t pos_stride = ws.pos_stride();
    if ((PART & DE_POS_PART) != 0 && dE_out && bid == 0 && threadIdx.x == 0)
        dE_out[DeWs::POS_MASK] = pos_out ? (float)((1 << DE_POS_MLP_CLASSES) - 1) : 0.f;
    const int lm_rows = bwd_blocks_of(n);            // level_max rows the scatter reads
    // split passes' stash (ncn_field_bwd_stash_floats): [groups][64] operand tiles, then [groups][16]
    // fp32 row-0 elements (capacity groups: the layout does not depend on the device count)
    v4* stq = (v4*)stash;
    float* sth0 = stash ? stash + ((n + 15) / 16) * 128 : nullptr;
    const int64_t n_cap = n;
    if (n_dev) n = min<int64_t>(n, *n_dev);
    constexpr bool SIGONLY = PART == BWD_SIGMA;
    constexpr int NF32 = BwdLds<T, PART>::NF32, NF16 = BwdLds<T, PART>::NF16, NX = BwdLds<T, PART>::NX;
    SG_TREAL(6);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t n_groups = (n + 15) / 16;
    const int64_t stride = (int64_t)nblk * BWD_WAVES;
    int64_t base = (int64_t)bid * BWD_WAVES;  // first group of this workgroup's step
    BwdIn<T> nxt;
    // (sigma pass: the first step's loads leave before the fragments are staged, so the two latencies
    // overlap; the other passes keep their registers free until the loop)
    if constexpr (SIGONLY) {
        if (base + wid < n_groups)
            bwd_load<T, PART>(nxt, base + wid, n, lane, enc_cache, dirs, dL_dsig, dL_dsig2, dL_drgb, stq, sth0, order, S,
                              pos_src);
    }
    {
        const v8* w32 = (const v8*)wpacked;
        const v4* w16 = (const v4*)(wpacked + N_FRAG32 * 512);
        for (int i = threadIdx.x; i < NF32 * 64; i += BWD_THREADS) {
            const int f = i >> 6;  // (sigma pass: B_L1 packed behind F_L2)
            F32s[i] = w32[(SIGONLY && f >= F_L3 ? f + (B_L1 - F_L3) : f) * 64 + (i & 63)];
        }
        for (int i = threadIdx.x; i < NF16 * 64; i += BWD_THREADS) F16s[i] = w16[(SIGONLY ? B_L2 * 64 : 0) + i];
    }
    if constexpr (PART == BWD_RGB) {  // the sigma pass max-reduces into the level_max rows: zero them
        if (bid == 0 && level_max)
            for (int i = threadIdx.x; i < lm_rows * 16; i += BWD_THREADS) level_max[i] = 0.f;
    }
    DinCtx<T> din = {nullptr, order, dL_ddirs};
    if constexpr (DIN) {
        __shared__ __attribute__((aligned(16))) T W3d[3 * 64];  // W3[j][k] of the fp32 masters at [k][j]
        for (int i = threadIdx.x; i < 3 * 64; i += BWD_THREADS) W3d[i] = (T)w_master[W3_OFF + (i & 63) * 32 + (i >> 6)];
        din.w3d = W3d;
        // the rows past the device count leave as zeros
        for (int64_t i = 3 * n + (int64_t)bid * BWD_THREADS + threadIdx.x; i < 3 * n_cap;
             i += (int64_t)nblk * BWD_THREADS)
            dL_ddirs[i] = 0.f;
    }
    __syncthreads();
    float4_t acc[5];
#pragma unroll
    for (int t = 0; t < 5; t++) acc[t] = zero4();
    float lm[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (!SIGONLY) {
        if (base + wid < n_groups)
            bwd_load<T, PART>(nxt, base + wid, n, lane, enc_cache, dirs, dL_dsig, dL_dsig2, dL_drgb, stq, sth0, order, S,
                              pos_src);
    }
    FragsSigmaReg<T> FR;  // (sigma pass) the K=32 fragments in registers for every group of the workgroup
    if constexpr (SIGONLY) {
        FragsSigma<T> Fl;
        Fl.f32 = F32s;
        Fl.f16 = F16s;
        FR.load(Fl, lane);
    }
    SG_TREAL(7);
    for (; base < n_groups; base += stride) {
        const int64_t grp = base + wid;
        const int ng = (int)min<int64_t>(BWD_WAVES, n_groups - base);
        const BwdIn<T> cur = nxt;
        SG_TNOW(g0);
        SG_TWAIT();  // (diagnostic: this step's prefetched loads, and the last step's dE stores, have landed)
        SG_TNOW(g1);
        if (grp + stride < n_groups)
            bwd_load<T, PART>(nxt, grp + stride, n, lane, enc_cache, dirs, dL_dsig, dL_dsig2, dL_drgb, stq, sth0, order,
                              S, pos_src);
        if (grp < n_groups) {
            if ((PART & DE_POS_PART) != 0 && pos_out && (lane >> 4) < DE_POS_MLP_CLASSES && grp * 16 + (lane & 15) < n) {
                const int cls = lane >> 4;
                float* po = pos_out + DeWs::class_offset(cls, pos_stride) + 3 * sc_perm(grp * 16 + (lane & 15), cls);
                po[0] = cur.px; po[1] = cur.py; po[2] = cur.pz;
            }
            if constexpr (SIGONLY) {
                bwd_group<T, PART, DIN>(FR, X + wid * NX * 256, cur, grp, n, n_stride, lane, dE_pairs, lm, inv_S, stq,
                                        sth0, &din);
            } else {
                Frags<T> F;
                const int z = opaque_zero();
                F.f32 = F32s + z;
                F.f16 = F16s + z;
                bwd_group<T, PART, DIN>(F, X + wid * NX * 256, cur, grp, n, n_stride, lane, dE_pairs, lm, inv_S, stq,
                                        sth0, &din);
            }
        }
        SG_TNOW(g2);
        lds_barrier();  // (the dE stores and the next step's loads stay in flight)
        SG_TNOW(g3);
        if constexpr (DIN) {
            // The transposed LDS reads of phase 2 must run with EXEC all ones (x_get): the group count
            // and the wave index are uniform, but the DIN instantiations' register allocation (the
            // one-pass form's; the rgb part's takes the same operands) keeps them in vector registers,
            // and a zero half of x_pair then becomes a read under EXEC = 0, which returns the stale
            // tile.  As scalars they are branches again.
            bwd_dw<T, PART>(X, __builtin_amdgcn_readfirstlane(ng), __builtin_amdgcn_readfirstlane(wid), lane, acc);
        } else
            bwd_dw<T, PART>(X, ng, wid, lane, acc);
        SG_TNOW(g4);
        lds_barrier();
        SG_TNOW(g5);
        SG_TADD(0, g0, g1);
        SG_TADD(1, g1, g2);
        SG_TADD(2, g2, g3);
        SG_TADD(3, g3, g4);
        SG_TADD(4, g4, g5);
        SG_TADD(5, 0ull, 1ull);
    }
    SG_TREAL(8);
    bwd_store_dw<PART>(slab + (int64_t)bid * NCN_FIELD_NW, wid, lane, acc, inv_S);
    if constexpr (PART == BWD_RGB) return;  // (no encoding gradient in the rgb pass: lmw is never allocated)
    // level maxima: the 16 lanes of a row (same g) share their 4 levels; the row leaders of the 8
    // waves meet in LDS and the workgroup writes its row of level_max [blocks][16] (no atomics: the
    // scatter reduces the rows)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float m = lm[i];
        m = fmaxf(m, dpp_f<0x128, 0xF>(0.f, m));  // row_ror 8
        m = fmaxf(m, dpp_f<0x124, 0xF>(0.f, m));
        m = fmaxf(m, dpp_f<0x122, 0xF>(0.f, m));
        m = fmaxf(m, dpp_f<0x121, 0xF>(0.f, m));
        lm[i] = m;
    }
    __shared__ float lmw[BWD_WAVES][16];
    if ((lane & 15) == 0) {
        const int g = lane >> 4;
        lmw[wid][2 * g] = lm[0];
        lmw[wid][2 * g + 1] = lm[1];
        lmw[wid][8 + 2 * g] = lm[2];
        lmw[wid][9 + 2 * g] = lm[3];
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        float m = 0.f;
#pragma unroll
        for (int w = 0; w < BWD_WAVES; w++) m = fmaxf(m, lmw[w][threadIdx.x]);
        if constexpr (PART == BWD_SIGMA)  // (any grid size: rows zeroed by the rgb pass; m >= 0, so the
            // IEEE order is the unsigned order of the bits)
            atomicMax((unsigned*)&level_max[(bid % lm_rows) * 16 + threadIdx.x], __float_as_uint(m));
        else
            level_max[bid * 16 + threadIdx.x] = m;
    }
    // a capped grid (ncn_field_bwd_mlp_part's n_blocks) leaves the scatter's remaining rows neutral
    if (PART == BWD_ALL && bid == 0)
        for (int i = nblk * 16 + threadIdx.x; i < lm_rows * 16; i += BWD_THREADS) level_max[i] = 0.f;
    SG_TREAL(9);
}

// (the sigma pass runs two workgroups per CU: 4 waves per SIMD, so at most 128 VGPRs)
template <typename T, int PART = BWD_ALL, bool DIN = false>
__global__ __launch_bounds__(BWD_THREADS, PART == BWD_SIGMA ? 4 : 2) void field_bwd_kernel(
    const float* __restrict__ dirs, int64_t n, const int32_t* __restrict__ n_dev, const uint16_t* __restrict__ wpacked,
    const typename Mfma<T>::v8* __restrict__ enc_cache, const float* __restrict__ dL_dsig,
    const float* __restrict__ dL_drgb, const float* __restrict__ loss_scale, float* __restrict__ dE_out,
    float* __restrict__ slab, float* __restrict__ level_max, const int32_t* __restrict__ order,
    const float* __restrict__ dL_dsig2 = nullptr, float* __restrict__ stash = nullptr,
    const float* __restrict__ xyzs = nullptr, const float* __restrict__ w_master = nullptr,
    float* __restrict__ dL_ddirs = nullptr) {
    typedef BwdLds<T, PART> Lds;
    __shared__ typename Mfma<T>::v8 F32s[Lds::NF32 * 64];
    __shared__ typename Mfma<T>::v4 F16s[Lds::NF16 * 64];
    __shared__ __attribute__((aligned(16))) uint16_t X[BWD_WAVES * Lds::NX * 256];
    field_bwd_body<T, PART, DIN>(F32s, F16s, X, (int)blockIdx.x, (int)gridDim.x, nullptr, dirs, n, n_dev, wpacked, enc_cache,
                                 dL_dsig, dL_drgb, loss_scale, dE_out, slab, level_max, order, dL_dsig2, stash, xyzs,
                                 w_master, dL_ddirs);
}

// Sum of the per-workgroup dW slabs: blockIdx.y takes a chunk of slabs (coalesced 1 KB rows),
// chunk partials are added with f32 atomics (gw accumulates, like every .grad).
constexpr int WRED_CHUNK = 16;
// (nb_sigma rows of the sigma_net weights W1, W2 and nb_rgb rows of the rgb_net's: the split
// backward's two passes run on grids of their own)
inline __global__ void reduce_wgrad_kernel(const float* __restrict__ slab, int nb_sigma, int nb_rgb, float* __restrict__ gw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NCN_FIELD_NW) return;
    const int nb = i < W3_OFF ? nb_sigma : nb_rgb;
    const int b0 = blockIdx.y * WRED_CHUNK, b1 = min(nb, b0 + WRED_CHUNK);
    if (b0 >= b1) return;
    float s = 0.f;
    for (int b = b0; b < b1; b++) s += slab[(int64_t)b * NCN_FIELD_NW + i];
    atomicAdd(gw + i, s);
}
}  // namespace ncn
