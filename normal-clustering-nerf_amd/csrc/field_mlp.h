// The field's MLPs on MFMA fragments: operand traits, weight packing, sigma_net and rgb_net forward.
#pragma once
#include "common.h"
#include "../../include/ncnerf.h"
namespace ncn {
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef short short4_t __attribute__((ext_vector_type(4)));

// MFMA operand traits: T = _Float16 or __bf16; v4 = one K=16 / half a K=32 fragment, v8 = K=32.
template <typename T> struct Mfma;
template <> struct Mfma<_Float16> {
    static constexpr bool f16 = true;
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    typedef _Float16 v8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ float4_t k32(v8 a, v8 b, float4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ float4_t k16(v4 a, v4 b, float4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mfma<__bf16> {
    static constexpr bool f16 = false;
    typedef __bf16 v4 __attribute__((ext_vector_type(4)));
    typedef __bf16 v8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ float4_t k32(v8 a, v8 b, float4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ float4_t k16(v4 a, v4 b, float4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
    }
};

__device__ __forceinline__ float4_t zero4() { return float4_t{0.f, 0.f, 0.f, 0.f}; }
template <typename T>
__device__ __forceinline__ typename Mfma<T>::v4 cvt4(float4_t v) {  // round to the operand type (RNE)
    typename Mfma<T>::v4 h;
#pragma unroll
    for (int i = 0; i < 4; i++) h[i] = (T)v[i];
    return h;
}
template <typename T>
__device__ __forceinline__ typename Mfma<T>::v4 relu4(float4_t v) {
    typename Mfma<T>::v4 h;
#pragma unroll
    for (int i = 0; i < 4; i++) h[i] = (T)fmaxf(v[i], 0.0f);
    return h;
}
// ReLU backward on a gradient tile: keep v where the saved (rounded) activation is > 0
template <typename T>
__device__ __forceinline__ typename Mfma<T>::v4 relu_mask4(float4_t v, typename Mfma<T>::v4 x) {
    typename Mfma<T>::v4 h;
#pragma unroll
    for (int i = 0; i < 4; i++) h[i] = (float)x[i] > 0.0f ? (T)v[i] : (T)0.0f;
    return h;
}
template <typename V8, typename V4>
__device__ __forceinline__ V8 cat8(V4 a, V4 b) {
    return V8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// ---- packed weight fragments ----
// K=32 fragments (64 lanes x 8 values = 1 KB; lane (g,r) element j = A[row r][k phi(g,j)])
// forward (A = W, rows = out, K = in)
constexpr int F_L1 = 0;    // [t 0..3]          W1[16t+r][phi]
constexpr int F_L2 = 4;    // [s 0..1]          W2[r][32s+phi]
constexpr int F_L3 = 6;    // [t 0..3]          W3[16t+r][psi]   (psi: the padded-input order, below)
constexpr int F_L4 = 10;   // [t 0..3][s 0..1]  W4[16t+r][32s+phi]
constexpr int F_L5 = 18;   // [s 0..1]          W5[r][32s+phi]   (all 16 padded output rows)
constexpr int N_FWD32 = 20;
// backward (A = W^T, rows = in, K = out)
constexpr int B_L4 = 20;   // [t 0..3][s 0..1]  W4[32s+phi][16t+r]
constexpr int B_L3 = 28;   // [s 0..1]          W3[32s+phi][3+r]   (rows = h only)
constexpr int B_L1 = 30;   // [t 0..1][s 0..1]  W1[32s+phi][16t+r]
constexpr int N_FRAG32 = 34;
// K=16 fragments (64 lanes x 4 values = 512 B; lane (g,r) element j = A[row r][k 4g+j]) of the two
// products whose K is a 16-wide layer output (the K=32 form would be half zeros)
constexpr int B_L5 = 0;    // [t 0..3]          W5[4g+j][16t+r]
constexpr int B_L2 = 4;    // [t 0..3]          W2[4g+j][16t+r]
constexpr int N_FRAG16 = 8;
constexpr int PACKED_HALVES = N_FRAG32 * 512 + N_FRAG16 * 256;
static_assert(PACKED_HALVES == NCN_FIELD_PACKED_HALVES, "packed size");

// master weight offsets (floats) inside the concatenated fp32 buffer (tcnn's padded shapes)
constexpr int W1_OFF = 0, W2_OFF = W1_OFF + 64 * 32, W3_OFF = W2_OFF + 16 * 64, W4_OFF = W3_OFF + 64 * 32,
              W5_OFF = W4_OFF + 64 * 64, W_TOTAL = W5_OFF + 16 * 64;
static_assert(W_TOTAL == NCN_FIELD_NW, "weights size");

__host__ __device__ constexpr int phi(int g, int j) { return j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4); }
// rgb_net input index of K element (g,j) of the layer-3 B operand [h tile | d,pad tile]:
// j < 4: h feature 4g+j = input 3+4g+j; j >= 4: q = 4g+j-4, input q (d, q < 3) or 16+q (padding)
__host__ __device__ constexpr int psi(int g, int j) {
    return j < 4 ? 3 + 4 * g + j : ((4 * g + j - 4) < 3 ? (4 * g + j - 4) : 16 + (4 * g + j - 4));
}

// index into the concatenated master weights of packed element (f, lane, j)
__host__ __device__ constexpr int frag32_index(int f, int lane, int j) {
    const int g = lane >> 4, r = lane & 15, k = phi(g, j);
    if (f < F_L2) return W1_OFF + (16 * (f - F_L1) + r) * 32 + k;
    if (f < F_L3) return W2_OFF + r * 64 + 32 * (f - F_L2) + k;
    if (f < F_L4) return W3_OFF + (16 * (f - F_L3) + r) * 32 + psi(g, j);
    if (f < F_L5) return W4_OFF + (16 * ((f - F_L4) >> 1) + r) * 64 + 32 * ((f - F_L4) & 1) + k;
    if (f < B_L4) return W5_OFF + r * 64 + 32 * (f - F_L5) + k;
    if (f < B_L3) return W4_OFF + (32 * ((f - B_L4) & 1) + k) * 64 + 16 * ((f - B_L4) >> 1) + r;
    if (f < B_L1) return W3_OFF + (32 * (f - B_L3) + k) * 32 + 3 + r;
    return W1_OFF + (32 * ((f - B_L1) & 1) + k) * 32 + 16 * ((f - B_L1) >> 1) + r;
}
__host__ __device__ constexpr int frag16_index(int f, int lane, int j) {
    const int g = lane >> 4, r = lane & 15, k = 4 * g + j;
    return f < B_L2 ? W5_OFF + k * 64 + 16 * (f - B_L5) + r : W2_OFF + k * 64 + 16 * (f - B_L2) + r;
}
__device__ float frag32_value(const float* __restrict__ W, int f, int lane, int j) { return W[frag32_index(f, lane, j)]; }
__device__ float frag16_value(const float* __restrict__ W, int f, int lane, int j) { return W[frag16_index(f, lane, j)]; }

// packed position -> master weight index (ncn_field_pack_map)
inline __global__ void pack_map_kernel(int32_t* __restrict__ src) {
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f < N_FRAG32) {
        for (int j = 0; j < 8; j++) src[(f * 64 + lane) * 8 + j] = frag32_index(f, lane, j);
    } else {
        const int f16 = f - N_FRAG32;
        for (int j = 0; j < 4; j++) src[N_FRAG32 * 512 + (f16 * 64 + lane) * 4 + j] = frag16_index(f16, lane, j);
    }
}

template <typename T>
__global__ void pack_weights_kernel(const float* __restrict__ W, T* __restrict__ out) {
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f < N_FRAG32) {
#pragma unroll
        for (int j = 0; j < 8; j++) out[(f * 64 + lane) * 8 + j] = (T)frag32_value(W, f, lane, j);
    } else {
        const int f16 = f - N_FRAG32;
#pragma unroll
        for (int j = 0; j < 4; j++) out[N_FRAG32 * 512 + (f16 * 64 + lane) * 4 + j] = (T)frag16_value(W, f16, lane, j);
    }
}

// LDS fragment tables: K=32 fragments as v8 per lane, then the K=16 ones as v4 per lane
template <typename T>
struct Frags {
    typedef typename Mfma<T>::v4 v4;
    typedef typename Mfma<T>::v8 v8;
    const v8* f32;
    const v4* f16;
    __device__ __forceinline__ v8 a32(int f, int lane) const { return f32[f * 64 + lane]; }
    __device__ __forceinline__ v4 a16(int f, int lane) const { return f16[f * 64 + lane]; }
};
// The sigma_net fragments alone (the split backward's sigma pass, compact LDS): F_L1, F_L2 at
// their indices, B_L1 packed right behind them; B_L2 as the only fp16 fragments.
template <typename T>
struct FragsSigma : Frags<T> {
    __device__ __forceinline__ typename Mfma<T>::v8 a32(int f, int lane) const {
        return this->f32[(f >= B_L1 ? f - (B_L1 - F_L3) : f) * 64 + lane];
    }
    __device__ __forceinline__ typename Mfma<T>::v4 a16(int f, int lane) const {
        return this->f16[(f - B_L2) * 64 + lane];
    }
};
constexpr int N_SIG32 = F_L3 + 4, N_SIG16 = 4;  // F_L1, F_L2, B_L1 / B_L2
// The sigma pass's fragments with F_L1 and B_L1 (8 K=32 fragments, 32 VGPRs) held in registers for
// the whole kernel (the indices are constants once the layer loops are unrolled): no LDS read in
// front of 8 of a group's 14 MFMAs.  F_L2 and the four K=16 fragments stay in LDS: the pass has 128
// VGPRs at two workgroups per CU, and the unrolled phase 2 (bwd_dw) needs the rest (with all ten
// K=32 fragments in registers the fp16 pass spilled: DESIGN section 7, round 7 findings).
template <typename T>
struct FragsSigmaReg {
    typename Mfma<T>::v8 r32[N_SIG32];  // (F_L2's two entries unused)
    const typename Mfma<T>::v8* f32;
    const typename Mfma<T>::v4* f16;
    __device__ __forceinline__ void load(const FragsSigma<T>& F, int lane) {
#pragma unroll
        for (int f = 0; f < N_SIG32; f++)
            if (f < F_L2 || f >= F_L3) r32[f] = F.f32[f * 64 + lane];
        f32 = F.f32;
        f16 = F.f16;
    }
    __device__ __forceinline__ typename Mfma<T>::v8 a32(int f, int lane) const {
        if (f >= F_L2 && f < F_L3) return f32[f * 64 + lane];
        return r32[f >= B_L1 ? f - (B_L1 - F_L3) : f];
    }
    __device__ __forceinline__ typename Mfma<T>::v4 a16(int f, int lane) const { return f16[(f - B_L2) * 64 + lane]; }
};

// Shared per-group forward (16 samples).  Produces every intermediate the backward needs.
template <typename T>
struct FwdState {
    typedef typename Mfma<T>::v4 v4;
    v4 x2[4];       // relu(H1) tiles (B operands of L2)
    float4_t h;     // sigma_net output tile (rows 4g..4g+3)
    v4 x3h, x3d;    // L3 B operand halves: h tile, [d, 1-padding] tile
    v4 x4[4];       // relu(G1)
    v4 x5[4];       // relu(G2)
    float4_t out;   // rgb pre-activation tile (rows 0..2 valid on g==0)
};

template <typename T, typename FR>
__device__ __forceinline__ void mlp_sigma(const FR& F, int lane, typename Mfma<T>::v8 e, FwdState<T>& st) {
    typedef Mfma<T> M;
    typedef typename M::v8 v8;
#pragma unroll
    for (int t = 0; t < 4; t++) st.x2[t] = relu4<T>(M::k32(F.a32(F_L1 + t, lane), e, zero4()));
    float4_t h = M::k32(F.a32(F_L2, lane), cat8<v8>(st.x2[0], st.x2[1]), zero4());
    st.h = M::k32(F.a32(F_L2 + 1, lane), cat8<v8>(st.x2[2], st.x2[3]), h);
}

template <typename T>
__device__ __forceinline__ void mlp_rgb(const Frags<T>& F, int lane, float dnx, float dny, float dnz, FwdState<T>& st) {
    typedef Mfma<T> M;
    typedef typename M::v8 v8;
    const int g = lane >> 4;
    st.x3h = cvt4<T>(st.h);
    // [d, 1-padding]: element i of lane group g is padded-input q = 4g+i: d[q] for q < 3, else 1.0
    st.x3d = cvt4<T>(float4_t{g == 0 ? dnx : 1.f, g == 0 ? dny : 1.f, g == 0 ? dnz : 1.f, 1.f});
    const v8 b3 = cat8<v8>(st.x3h, st.x3d);
#pragma unroll
    for (int t = 0; t < 4; t++) st.x4[t] = relu4<T>(M::k32(F.a32(F_L3 + t, lane), b3, zero4()));
    const v8 b4a = cat8<v8>(st.x4[0], st.x4[1]), b4b = cat8<v8>(st.x4[2], st.x4[3]);
#pragma unroll
    for (int t = 0; t < 4; t++)
        st.x5[t] = relu4<T>(M::k32(F.a32(F_L4 + 2 * t + 1, lane), b4b, M::k32(F.a32(F_L4 + 2 * t, lane), b4a, zero4())));
    const float4_t o = M::k32(F.a32(F_L5, lane), cat8<v8>(st.x5[0], st.x5[1]), zero4());
    st.out = M::k32(F.a32(F_L5 + 1, lane), cat8<v8>(st.x5[2], st.x5[3]), o);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }
}  // namespace ncn
