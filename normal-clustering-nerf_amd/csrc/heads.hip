// libncnerf.so — the semantic / normal heads of NGPMT (include/ncnerf_heads.h): one generic kernel pair
// for tcnn's FullyFusedMLP(16 -> 64 -> 64 -> n_out) on the field's MFMA helpers, and the compositing of
// the heads' channels through the compositor's weights.
//
// Both head kernels recompute h from the field's encoding cache with the field's own mlp_sigma and
// packed W1 / W2, then run the head on 16-sample groups exactly as the field runs rgb_net: weights
// as A operands (rows = outputs), activations as B operands (columns = samples), an accumulator
// tile (lane (g, r): rows 4g..4g+3 of sample r) rounded in place into the next layer's B operand.
// The backward is field_bwd_mlp.h's two-phase form: phase 1, every wave on its own group, forward
// recompute, the three transposed products, dL/dh added into the split backward's stash, and the 20
// operand tiles of the weight gradient into the LDS exchange area; phase 2, wave w accumulates the 4
// dW tiles it owns over the step's groups.  Groups are dealt to workgroups and waves by index, every
// sum has a fixed order, nothing is atomic: two runs give the same bits.
#include <algorithm>
#include "field_bwd_mlp.h"
#include "../../include/ncnerf_heads.h"

namespace ncn {
// ---- packed fragments of one head (the K=32 / K=16 forms of field_mlp.h) ----
// K=32: forward Wb [t][s], Wc [ot][s]; backward (A = W^T) Wb [t][s], Wa [s]
constexpr int HF_B = 0;    // [t 0..3][s 0..1]   Wb[16t+r][32s+phi]
constexpr int HF_C = 8;    // [ot 0..2][s 0..1]  Wc[16ot+r][32s+phi]
constexpr int HB_B = 14;   // [t 0..3][s 0..1]   Wb[32s+phi][16t+r]
constexpr int HB_A = 22;   // [s 0..1]           Wa[32s+phi][r]
constexpr int N_H32 = 24, N_HFWD32 = HB_B;
// K=16: forward Wa [t]; backward Wc [ot][t]
constexpr int HF_A = 0;    // [t 0..3]           Wa[16t+r][4g+j]
constexpr int HB_C = 4;    // [ot 0..2][t 0..3]  Wc[16ot+4g+j][16t+r]
constexpr int N_H16 = 16, N_HFWD16 = HB_C;
constexpr int HEAD_PACKED = N_H32 * 512 + N_H16 * 256;
static_assert(HEAD_PACKED == NCN_HEAD_PACKED_HALVES, "packed size");
constexpr int WA_OFF = 0, WB_OFF = 64 * 16, WC_OFF = WB_OFF + 64 * 64;
constexpr int HEAD_MAX_TILES = (NCN_HEAD_MAX_OUT + 15) / 16;
static_assert(HEAD_MAX_TILES == 3 && NCN_EXTRA_MAX_CH <= WAVE, "three output tiles, a lane per channel");

// master index of packed element (f, lane, j), or -1 for an output tile the head does not have
__host__ __device__ constexpr int head32_index(int f, int lane, int j, int nt) {
    const int g = lane >> 4, r = lane & 15, k = phi(g, j);
    if (f < HF_C) return WB_OFF + (16 * ((f - HF_B) >> 1) + r) * 64 + 32 * ((f - HF_B) & 1) + k;
    if (f < HB_B) return ((f - HF_C) >> 1) < nt ? WC_OFF + (16 * ((f - HF_C) >> 1) + r) * 64 + 32 * ((f - HF_C) & 1) + k : -1;
    if (f < HB_A) return WB_OFF + (32 * ((f - HB_B) & 1) + k) * 64 + 16 * ((f - HB_B) >> 1) + r;
    return WA_OFF + (32 * (f - HB_A) + k) * 16 + r;
}
__host__ __device__ constexpr int head16_index(int f, int lane, int j, int nt) {
    const int g = lane >> 4, r = lane & 15, k = 4 * g + j;
    if (f < HB_C) return WA_OFF + (16 * (f - HF_A) + r) * 16 + k;
    return ((f - HB_C) >> 2) < nt ? WC_OFF + (16 * ((f - HB_C) >> 2) + k) * 64 + 16 * ((f - HB_C) & 3) + r : -1;
}

template <typename T>
__global__ void head_pack_kernel(const float* __restrict__ W, int nt, T* __restrict__ out) {
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f < N_H32) {
        for (int j = 0; j < 8; j++) {
            const int i = head32_index(f, lane, j, nt);
            out[(f * 64 + lane) * 8 + j] = i >= 0 ? (T)W[i] : (T)0.0f;
        }
    } else {
        const int f16 = f - N_H32;
        for (int j = 0; j < 4; j++) {
            const int i = head16_index(f16, lane, j, nt);
            out[N_H32 * 512 + (f16 * 64 + lane) * 4 + j] = i >= 0 ? (T)W[i] : (T)0.0f;
        }
    }
}

// The head's forward on one group, from the field's h tile: the B operands of the three layers.
template <typename T>
struct HeadState {
    typedef typename Mfma<T>::v4 v4;
    v4 xh;      // h tile rounded (the field's x3h)
    v4 xa[4];   // relu(Wa h)
    v4 xc[4];   // relu(Wb xa)
};
template <typename T>
__device__ __forceinline__ void head_hidden(const Frags<T>& H, int lane, float4_t h, HeadState<T>& hs) {
    typedef Mfma<T> M;
    typedef typename M::v8 v8;
    hs.xh = cvt4<T>(h);
#pragma unroll
    for (int t = 0; t < 4; t++) hs.xa[t] = relu4<T>(M::k16(H.a16(HF_A + t, lane), hs.xh, zero4()));
    const v8 ba = cat8<v8>(hs.xa[0], hs.xa[1]), bb = cat8<v8>(hs.xa[2], hs.xa[3]);
#pragma unroll
    for (int t = 0; t < 4; t++)
        hs.xc[t] = relu4<T>(M::k32(H.a32(HF_B + 2 * t + 1, lane), bb, M::k32(H.a32(HF_B + 2 * t, lane), ba, zero4())));
}

// Forward: grid-stride over 16-sample groups, one group per wave per step.
constexpr int HEAD_FWD_THREADS = 256;
template <typename T>
__global__ __launch_bounds__(HEAD_FWD_THREADS) void head_fwd_kernel(
    const typename Mfma<T>::v8* __restrict__ enc_cache, int64_t n, const int32_t* __restrict__ n_dev,
    const uint16_t* __restrict__ fpacked, const uint16_t* __restrict__ hpacked, int n_out, float* __restrict__ out) {
    typedef Mfma<T> M;
    typedef typename M::v4 v4;
    typedef typename M::v8 v8;
    __shared__ v8 Fs[F_L3 * 64];         // the field's F_L1, F_L2
    __shared__ v8 H32s[N_HFWD32 * 64];   // HF_B, HF_C
    __shared__ v4 H16s[N_HFWD16 * 64];   // HF_A
    if (n_dev) n = min<int64_t>(n, *n_dev);
    for (int i = threadIdx.x; i < F_L3 * 64; i += HEAD_FWD_THREADS) Fs[i] = ((const v8*)fpacked)[i];
    for (int i = threadIdx.x; i < N_HFWD32 * 64; i += HEAD_FWD_THREADS) H32s[i] = ((const v8*)hpacked)[i];
    for (int i = threadIdx.x; i < N_HFWD16 * 64; i += HEAD_FWD_THREADS) H16s[i] = ((const v4*)(hpacked + N_H32 * 512))[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    const int nt = (n_out + 15) >> 4;
    const int64_t n_groups = (n + 15) / 16;
    const int64_t wave0 = (int64_t)blockIdx.x * (HEAD_FWD_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (HEAD_FWD_THREADS / 64);
    for (int64_t grp = wave0; grp < n_groups; grp += n_waves) {
        const int z = opaque_zero();  // fragments re-read from LDS every group (not hoisted)
        Frags<T> F, H;
        F.f32 = Fs + z;
        F.f16 = nullptr;
        H.f32 = H32s + z;
        H.f16 = H16s + z;
        FwdState<T> st;
        mlp_sigma<T>(F, lane, enc_cache[grp * 64 + lane], st);
        HeadState<T> hs;
        head_hidden<T>(H, lane, st.h, hs);
        const v8 ca = cat8<v8>(hs.xc[0], hs.xc[1]), cb = cat8<v8>(hs.xc[2], hs.xc[3]);
        const int64_t s = grp * 16 + r;
        for (int ot = 0; ot < nt; ot++) {
            const float4_t o = M::k32(H.a32(HF_C + 2 * ot + 1, lane), cb, M::k32(H.a32(HF_C + 2 * ot, lane), ca, zero4()));
            if (s < n) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int row = 16 * ot + 4 * g + i;
                    if (row < n_out) out[s * n_out + row] = o[i];
                }
            }
        }
    }
}

// The features alone (NGPMT.density(x, return_feat=True)): h (n, 16) fp32, the unrounded accumulators
// of sigma_net's last layer, from the encoding cache.
template <typename T>
__global__ __launch_bounds__(HEAD_FWD_THREADS) void head_feat_kernel(
    const typename Mfma<T>::v8* __restrict__ enc_cache, int64_t n, const int32_t* __restrict__ n_dev,
    const uint16_t* __restrict__ fpacked, float* __restrict__ h) {
    typedef typename Mfma<T>::v8 v8;
    __shared__ v8 Fs[F_L3 * 64];  // the field's F_L1, F_L2
    if (n_dev) n = min<int64_t>(n, *n_dev);
    for (int i = threadIdx.x; i < F_L3 * 64; i += HEAD_FWD_THREADS) Fs[i] = ((const v8*)fpacked)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    const int64_t n_groups = (n + 15) / 16;
    const int64_t wave0 = (int64_t)blockIdx.x * (HEAD_FWD_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (HEAD_FWD_THREADS / 64);
    for (int64_t grp = wave0; grp < n_groups; grp += n_waves) {
        Frags<T> F;
        F.f32 = Fs + opaque_zero();
        F.f16 = nullptr;
        FwdState<T> st;
        mlp_sigma<T>(F, lane, enc_cache[grp * 64 + lane], st);
        const int64_t s = grp * 16 + r;
        if (s < n) *(float4_t*)(h + s * 16 + 4 * g) = st.h;  // (rows 4g..4g+3 of sample s: 16-byte aligned)
    }
}

// Backward.  Exchange tiles per group: dW operands, A = dY^T, B = X^T (field_bwd_mlp.h x_put / x_get).
constexpr int HXAC = 0, HXBC = 3, HXAB = 7, HXBB = 11, HXAA = 15, HXBA = 19, N_HX = 20;

// (Its 118 KB of LDS — fragments 6 + 24 + 8 KB, the exchange area 80 KB — leave room for one workgroup
// per CU; the second launch-bounds argument, 2 waves per SIMD, is that one workgroup's 8 waves and
// only states the register budget, 256 VGPRs.)
template <typename T>
__global__ __launch_bounds__(BWD_THREADS, 2) void head_bwd_kernel(
    const typename Mfma<T>::v8* __restrict__ enc_cache, int64_t n, const int32_t* __restrict__ n_dev,
    const uint16_t* __restrict__ fpacked, const uint16_t* __restrict__ hpacked, int n_out,
    const float* __restrict__ dL_dout, const float* __restrict__ loss_scale, float* __restrict__ slab,
    float* __restrict__ stash) {
    typedef Mfma<T> M;
    typedef typename M::v4 v4;
    typedef typename M::v8 v8;
    __shared__ v8 Fs[F_L3 * 64];
    __shared__ v8 H32s[N_H32 * 64];
    __shared__ v4 H16s[N_H16 * 64];
    __shared__ __attribute__((aligned(16))) uint16_t X[BWD_WAVES * N_HX * 256];
    const float S = loss_scale ? *loss_scale * (M::f16 ? NCN_TCNN_LOSS_SCALE : 1.f) : 1.f, inv_S = 1.f / S;
    // the stash of ncn_field_bwd_mlp_part: [groups][64] operand tiles, then [groups][16] fp32 row-0 values
    v4* const stq = (v4*)stash;
    float* const sth0 = stash + ((n + 15) / 16) * 128;
    if (n_dev) n = min<int64_t>(n, *n_dev);
    for (int i = threadIdx.x; i < F_L3 * 64; i += BWD_THREADS) Fs[i] = ((const v8*)fpacked)[i];
    for (int i = threadIdx.x; i < N_H32 * 64; i += BWD_THREADS) H32s[i] = ((const v8*)hpacked)[i];
    for (int i = threadIdx.x; i < N_H16 * 64; i += BWD_THREADS) H16s[i] = ((const v4*)(hpacked + N_H32 * 512))[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    // (the transposed LDS reads of phase 2 run with EXEC all ones only under scalar branches)
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nt = (n_out + 15) >> 4;
    const int64_t n_groups = (n + 15) / 16;
    const int64_t stride = (int64_t)gridDim.x * BWD_WAVES;
    uint16_t* const Xw = X + wid * N_HX * 256;
    float4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = zero4();
    for (int64_t base = (int64_t)blockIdx.x * BWD_WAVES; base < n_groups; base += stride) {
        const int64_t grp = base + wid;
        const int ng = __builtin_amdgcn_readfirstlane((int)min<int64_t>(BWD_WAVES, n_groups - base));
        if (grp < n_groups) {
            const int z = opaque_zero();
            Frags<T> F, H;
            F.f32 = Fs + z;
            F.f16 = nullptr;
            H.f32 = H32s + z;
            H.f16 = H16s + z;
            const int64_t s = grp * 16 + r;
            FwdState<T> st;
            mlp_sigma<T>(F, lane, enc_cache[grp * 64 + lane], st);
            HeadState<T> hs;
            head_hidden<T>(H, lane, st.h, hs);
            // dY: the upstream gradient at the chain's scale, rows >= n_out and samples >= n zero
            v4 dY[HEAD_MAX_TILES];
#pragma unroll
            for (int ot = 0; ot < HEAD_MAX_TILES; ot++) {
                float4_t d = zero4();
                if (ot < nt && s < n) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int row = 16 * ot + 4 * g + i;
                        if (row < n_out) d[i] = dL_dout[s * n_out + row] * S;
                    }
                }
                dY[ot] = cvt4<T>(d);
                x_put(Xw + (HXAC + ot) * 256, lane, dY[ot]);
            }
            // last layer backward -> ReLU(xc) mask -> dDc; the padded tiles' fragments are zeros
            v4 dDc[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                float4_t a = zero4();
#pragma unroll
                for (int ot = 0; ot < HEAD_MAX_TILES; ot++)
                    if (ot < nt) a = M::k16(H.a16(HB_C + 4 * ot + t, lane), dY[ot], a);
                dDc[t] = relu_mask4<T>(a, hs.xc[t]);
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                x_put(Xw + (HXBC + t) * 256, lane, hs.xc[t]);
                x_put(Xw + (HXAB + t) * 256, lane, dDc[t]);
                x_put(Xw + (HXBB + t) * 256, lane, hs.xa[t]);
            }
            // middle layer backward -> ReLU(xa) mask -> dDa
            const v8 dca = cat8<v8>(dDc[0], dDc[1]), dcb = cat8<v8>(dDc[2], dDc[3]);
            v4 dDa[4];
#pragma unroll
            for (int t = 0; t < 4; t++)
                dDa[t] = relu_mask4<T>(
                    M::k32(H.a32(HB_B + 2 * t + 1, lane), dcb, M::k32(H.a32(HB_B + 2 * t, lane), dca, zero4())), hs.xa[t]);
#pragma unroll
            for (int t = 0; t < 4; t++) x_put(Xw + (HXAA + t) * 256, lane, dDa[t]);
            x_put(Xw + HXBA * 256, lane, hs.xh);
            // first layer backward -> dL/dh, added into the stash: fp32 sum, one rounding
            float4_t dh = M::k32(H.a32(HB_A, lane), cat8<v8>(dDa[0], dDa[1]), zero4());
            dh = M::k32(H.a32(HB_A + 1, lane), cat8<v8>(dDa[2], dDa[3]), dh);
            const v4 q = stq[grp * 64 + lane];
            stq[grp * 64 + lane] = cvt4<T>(float4_t{(float)q[0] + dh[0], (float)q[1] + dh[1], (float)q[2] + dh[2],
                                                    (float)q[3] + dh[3]});
            if (g == 0) sth0[grp * 16 + r] += dh[0];
        }
        lds_barrier();
        // phase 2: waves 0-3 own Wb's row block wid (4 tiles); waves 4-7 Wa's row block wid - 4 and
        // the column block wid - 4 of every Wc row block
        for (int q = 0; q < ng; q += 2) {
            if (wid < 4) {
                const v8 A = x_pair<T, N_HX>(X, q, ng, HXAB + wid, lane);
#pragma unroll
                for (int b = 0; b < 4; b++) acc[b] = M::k32(A, x_pair<T, N_HX>(X, q, ng, HXBB + b, lane), acc[b]);
            } else {
                acc[0] = M::k32(x_pair<T, N_HX>(X, q, ng, HXAA + wid - 4, lane), x_pair<T, N_HX>(X, q, ng, HXBA, lane), acc[0]);
                const v8 B = x_pair<T, N_HX>(X, q, ng, HXBC + wid - 4, lane);
#pragma unroll
                for (int ot = 0; ot < HEAD_MAX_TILES; ot++)
                    if (ot < nt) acc[1 + ot] = M::k32(x_pair<T, N_HX>(X, q, ng, HXAC + ot, lane), B, acc[1 + ot]);
            }
        }
        lds_barrier();
    }
    // the owned tiles (C layout: lane (g, r) = rows 4g+i, column r) into the workgroup's slab row
    float* const o = slab + (int64_t)blockIdx.x * NCN_HEAD_NW(n_out);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = 4 * g + i;
        if (wid < 4) {
#pragma unroll
            for (int b = 0; b < 4; b++) o[WB_OFF + (16 * wid + row) * 64 + 16 * b + r] = acc[b][i] * inv_S;
        } else {
            o[WA_OFF + (16 * (wid - 4) + row) * 16 + r] = acc[0][i] * inv_S;
#pragma unroll
            for (int ot = 0; ot < HEAD_MAX_TILES; ot++)
                if (ot < nt) o[WC_OFF + (16 * ot + row) * 64 + 16 * (wid - 4) + r] = acc[1 + ot][i] * inv_S;
        }
    }
}

// Sum of the slab rows in a fixed order: 64 weights x HRED_RUNS runs of consecutive rows per workgroup,
// then the runs in order; grad_w accumulates, like every .grad.
constexpr int HRED_RUNS = 16;
__global__ __launch_bounds__(64 * HRED_RUNS) void head_reduce_wgrad_kernel(const float* __restrict__ slab, int nb, int n_w,
                                                                          float* __restrict__ gw) {
    __shared__ float part[HRED_RUNS][64];
    const int j = threadIdx.x & 63, c = threadIdx.x >> 6, i = blockIdx.x * 64 + j;
    const int per = (nb + HRED_RUNS - 1) / HRED_RUNS, b0 = c * per, b1 = min(nb, b0 + per);
    float s = 0.f;
    if (i < n_w)
        for (int b = b0; b < b1; b++) s += slab[(int64_t)b * n_w + i];
    part[c][j] = s;
    __syncthreads();
    if (c == 0 && i < n_w) {
        float t = part[0][j];
#pragma unroll
        for (int k = 1; k < HRED_RUNS; k++) t += part[k][j];
        gw[i] += t;
    }
}

// ---- extra channels through the compositor's weights: a wave per ray ----
// A sample's n_ch channels take a segment of W lanes, W the power of two >= n_ch, so a wave works
// on P = 64 / W samples at once and its loads are runs of consecutive floats of raws.  Lane (p, c):
// channel c of the samples start + p, start + p + P, ...
constexpr int EX_THREADS = 256;
__device__ __forceinline__ int extra_seg_width(int n_ch) {  // (uniform)
    int w = 1;
    while (w < n_ch) w <<= 1;
    return w;
}
// Forward: every lane sums its samples in order, then the P sub-sums of a channel are added in p order.
__global__ __launch_bounds__(EX_THREADS) void composite_extra_fw_kernel(
    const float* __restrict__ ws, const float* __restrict__ raws, const int64_t* __restrict__ rays_a, int64_t n_rays,
    int64_t n_samples, int n_ch, float* __restrict__ rend) {
    const int64_t i = (int64_t)blockIdx.x * (EX_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n_rays) return;  // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int64_t ray = rays_a[3 * i], start = rays_a[3 * i + 1], cnt = rays_a[3 * i + 2];
    if (ray < 0 || ray >= n_rays) return;
    const int64_t s0 = max<int64_t>(start, 0), s1 = min<int64_t>(start + max<int64_t>(cnt, 0), n_samples);
    const int W = extra_seg_width(n_ch), P = 64 / W, p = lane / W, c = lane & (W - 1);
    float a = 0.f;
    if (c < n_ch)
        for (int64_t s = s0 + p; s < s1; s += P) a = fmaf(ws[s], raws[s * n_ch + c], a);
    float t = 0.f;
    for (int pp = 0; pp < P; pp++) t += shfl(a, pp * W + c);
    if (lane < n_ch) rend[ray * n_ch + lane] = t;
}

// Backward: dL_draws per lane; dL_dws = the sum of a segment's products by an xor butterfly inside the
// segment (a fixed order; the lanes past n_ch add zeros).
__global__ __launch_bounds__(EX_THREADS) void composite_extra_bw_kernel(
    const float* __restrict__ dL_drend, const float* __restrict__ ws, const float* __restrict__ raws,
    const int64_t* __restrict__ rays_a, int64_t n_rays, int64_t n_samples, int n_ch, float* __restrict__ dL_dws,
    float* __restrict__ dL_draws) {
    const int64_t i = (int64_t)blockIdx.x * (EX_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n_rays) return;  // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int64_t ray = rays_a[3 * i], start = rays_a[3 * i + 1], cnt = rays_a[3 * i + 2];
    if (ray < 0 || ray >= n_rays) return;
    const int64_t s0 = max<int64_t>(start, 0), s1 = min<int64_t>(start + max<int64_t>(cnt, 0), n_samples);
    const int W = extra_seg_width(n_ch), P = 64 / W, p = lane / W, c = lane & (W - 1);
    const float g = c < n_ch ? dL_drend[ray * n_ch + c] : 0.f;
    for (int64_t base = s0; base < s1; base += P) {  // (uniform trip count: every lane takes part in the butterfly)
        const int64_t s = base + p;
        const bool ok = c < n_ch && s < s1;
        float prod = 0.f;
        if (ok) {
            prod = g * raws[s * n_ch + c];
            dL_draws[s * n_ch + c] = g * ws[s];
        }
        for (int off = W >> 1; off >= 1; off >>= 1) prod += __shfl_xor(prod, off, WAVE);
        if (c == 0 && s < s1) dL_dws[s] = prod;
    }
}

template <typename T> struct HeadOperand { typedef T type; };
template <typename F>
static void with_head_operand(int precision, F&& f) {
    if (precision == NCN_PREC_F16) f(HeadOperand<_Float16>{});
    else f(HeadOperand<__bf16>{});
}
static int head_check(const char* name, int n_out, int precision) {
    NCN_REQUIRE(n_out >= 1 && n_out <= NCN_HEAD_MAX_OUT, hipErrorInvalidValue, "%s: n_out must lie in [1, %d] (got %d)",
                name, NCN_HEAD_MAX_OUT, n_out);
    NCN_REQUIRE(precision == NCN_PREC_F16 || precision == NCN_PREC_BF16, hipErrorInvalidValue,
                "%s: precision must be NCN_PREC_F16 or NCN_PREC_BF16", name);
    return 0;
}
static int extra_check(const char* name, int64_t n_samples, int n_ch) {
    NCN_REQUIRE(n_ch >= 1 && n_ch <= NCN_EXTRA_MAX_CH, hipErrorInvalidValue, "%s: n_ch must lie in [1, %d] (got %d)", name,
                NCN_EXTRA_MAX_CH, n_ch);
    NCN_REQUIRE(n_samples >= 0, hipErrorInvalidValue, "%s: n_samples must not be negative", name);
    return 0;
}
}  // namespace ncn
using namespace ncn;

extern "C" {
int ncn_head_packed_halves(int n_out) { return n_out >= 1 && n_out <= NCN_HEAD_MAX_OUT ? NCN_HEAD_PACKED_HALVES : -1; }

int ncn_head_pack_weights(const float* w_master, int n_out, uint16_t* packed, int precision, void* stream) {
    if (const int e = head_check("ncn_head_pack_weights", n_out, precision)) return e;
    NCN_REQUIRE(w_master && packed, hipErrorInvalidValue, "ncn_head_pack_weights: w_master and packed required");
    with_head_operand(precision, [&](auto op) {
        typedef typename decltype(op)::type T;
        hipLaunchKernelGGL(head_pack_kernel<T>, dim3(N_H32 + N_H16), dim3(64), 0, (hipStream_t)stream, w_master,
                           (n_out + 15) / 16, (T*)packed);
    });
    NCN_LAUNCH_CHECK("ncn_head_pack_weights");
    return 0;
}

int ncn_head_fwd(const uint16_t* enc_cache, int64_t n, const int32_t* n_dev, const uint16_t* field_weights_packed,
                 const uint16_t* head_packed, int n_out, int precision, float* out, void* stream) {
    if (const int e = head_check("ncn_head_fwd", n_out, precision)) return e;
    if (n <= 0) return 0;
    NCN_REQUIRE(enc_cache && field_weights_packed && head_packed && out, hipErrorInvalidValue,
                "ncn_head_fwd: enc_cache, field_weights_packed, head_packed and out required");
    NCN_REQUIRE((((uintptr_t)enc_cache | (uintptr_t)field_weights_packed | (uintptr_t)head_packed) & 15) == 0,
                hipErrorInvalidValue, "ncn_head_fwd: enc_cache / field_weights_packed / head_packed must be 16-byte aligned");
    const int64_t groups = (n + 15) / 16;
    const int grid = (int)std::min<int64_t>(std::max<int64_t>((groups + 3) / 4, 1), 2048);
    with_head_operand(precision, [&](auto op) {
        typedef typename decltype(op)::type T;
        hipLaunchKernelGGL(head_fwd_kernel<T>, dim3(grid), dim3(HEAD_FWD_THREADS), 0, (hipStream_t)stream,
                           (const typename Mfma<T>::v8*)enc_cache, n, n_dev, field_weights_packed, head_packed, n_out, out);
    });
    NCN_LAUNCH_CHECK("ncn_head_fwd");
    return 0;
}

int ncn_head_feat(const uint16_t* enc_cache, int64_t n, const int32_t* n_dev, const uint16_t* field_weights_packed,
                  int precision, float* h, void* stream) {
    if (const int e = head_check("ncn_head_feat", 1, precision)) return e;
    if (n <= 0) return 0;
    NCN_REQUIRE(enc_cache && field_weights_packed && h, hipErrorInvalidValue,
                "ncn_head_feat: enc_cache, field_weights_packed and h required");
    NCN_REQUIRE((((uintptr_t)enc_cache | (uintptr_t)field_weights_packed | (uintptr_t)h) & 15) == 0, hipErrorInvalidValue,
                "ncn_head_feat: enc_cache / field_weights_packed / h must be 16-byte aligned");
    const int64_t groups = (n + 15) / 16;
    const int grid = (int)std::min<int64_t>(std::max<int64_t>((groups + 3) / 4, 1), 2048);
    with_head_operand(precision, [&](auto op) {
        typedef typename decltype(op)::type T;
        hipLaunchKernelGGL(head_feat_kernel<T>, dim3(grid), dim3(HEAD_FWD_THREADS), 0, (hipStream_t)stream,
                           (const typename Mfma<T>::v8*)enc_cache, n, n_dev, field_weights_packed, h);
    });
    NCN_LAUNCH_CHECK("ncn_head_feat");
    return 0;
}

int ncn_head_bwd_blocks(int64_t n) { return bwd_blocks_of(n); }

int ncn_head_bwd(const uint16_t* enc_cache, int64_t n, const int32_t* n_dev, const uint16_t* field_weights_packed,
                 const uint16_t* head_packed, int n_out, int precision, const float* dL_dout, const float* loss_scale,
                 float* slab, float* dh_stash, void* stream) {
    if (const int e = head_check("ncn_head_bwd", n_out, precision)) return e;
    if (n <= 0) return 0;
    NCN_REQUIRE(enc_cache && field_weights_packed && head_packed && dL_dout && slab && dh_stash, hipErrorInvalidValue,
                "ncn_head_bwd: enc_cache, field_weights_packed, head_packed, dL_dout, slab and dh_stash required");
    NCN_REQUIRE((((uintptr_t)enc_cache | (uintptr_t)field_weights_packed | (uintptr_t)head_packed | (uintptr_t)dh_stash) & 15) == 0,
                hipErrorInvalidValue,
                "ncn_head_bwd: enc_cache / field_weights_packed / head_packed / dh_stash must be 16-byte aligned");
    with_head_operand(precision, [&](auto op) {
        typedef typename decltype(op)::type T;
        hipLaunchKernelGGL(head_bwd_kernel<T>, dim3(bwd_blocks_of(n)), dim3(BWD_THREADS), 0, (hipStream_t)stream,
                           (const typename Mfma<T>::v8*)enc_cache, n, n_dev, field_weights_packed, head_packed, n_out,
                           dL_dout, loss_scale, slab, dh_stash);
    });
    NCN_LAUNCH_CHECK("ncn_head_bwd");
    return 0;
}

int ncn_head_reduce_wgrad(const float* slab, int n_blocks, int n_w, float* grad_w, void* stream) {
    if (n_blocks <= 0 || n_w <= 0) return 0;
    NCN_REQUIRE(slab && grad_w, hipErrorInvalidValue, "ncn_head_reduce_wgrad: slab and grad_w required");
    hipLaunchKernelGGL(head_reduce_wgrad_kernel, dim3((unsigned)cdiv(n_w, 64)), dim3(64 * HRED_RUNS), 0, (hipStream_t)stream,
                       slab, n_blocks, n_w, grad_w);
    NCN_LAUNCH_CHECK("ncn_head_reduce_wgrad");
    return 0;
}

int ncn_composite_extra_fw(const float* ws, const float* raws, const int64_t* rays_a, int64_t n_rays, int64_t n_samples,
                           int n_ch, float* rend, void* stream) {
    if (const int e = extra_check("ncn_composite_extra_fw", n_samples, n_ch)) return e;
    if (n_rays <= 0) return 0;
    NCN_REQUIRE(ws && raws && rays_a && rend, hipErrorInvalidValue, "ncn_composite_extra_fw: ws, raws, rays_a and rend required");
    hipLaunchKernelGGL(composite_extra_fw_kernel, dim3((unsigned)cdiv(n_rays, EX_THREADS / 64)), dim3(EX_THREADS), 0,
                       (hipStream_t)stream, ws, raws, rays_a, n_rays, n_samples, n_ch, rend);
    NCN_LAUNCH_CHECK("ncn_composite_extra_fw");
    return 0;
}

int ncn_composite_extra_bw(const float* dL_drend, const float* ws, const float* raws, const int64_t* rays_a,
                           int64_t n_rays, int64_t n_samples, int n_ch, float* dL_dws, float* dL_draws, void* stream) {
    if (const int e = extra_check("ncn_composite_extra_bw", n_samples, n_ch)) return e;
    if (n_rays <= 0) return 0;
    NCN_REQUIRE(dL_drend && ws && raws && rays_a && dL_dws && dL_draws, hipErrorInvalidValue,
                "ncn_composite_extra_bw: dL_drend, ws, raws, rays_a, dL_dws and dL_draws required");
    hipLaunchKernelGGL(composite_extra_bw_kernel, dim3((unsigned)cdiv(n_rays, EX_THREADS / 64)), dim3(EX_THREADS), 0,
                       (hipStream_t)stream, dL_drend, ws, raws, rays_a, n_rays, n_samples, n_ch, dL_dws, dL_draws);
    NCN_LAUNCH_CHECK("ncn_composite_extra_bw");
    return 0;
}
}  // extern "C"
