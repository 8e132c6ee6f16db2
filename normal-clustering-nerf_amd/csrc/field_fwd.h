// Window sort, fused forward and the density pass's level-split encoding.
#pragma once
#include "field_grid.h"
#include "field_mlp.h"
namespace ncn {
// Processing order of the training step's samples (ncn_field_sort_windows).  The marcher packs
// samples ray by ray (the compositors need each ray's segment contiguous); the field does not care
// about order, and the table scatter of its backward aggregates the gradients of samples that share
// hash-grid corners — which, across the ~60 neighbouring rays of a patch, are samples at the same
// place in space, far apart in ray order.  So every window of SORT_W consecutive samples is sorted
// by the 30-bit Morton code of its normalised positions (10 bits per axis, the finest hash level's
// resolution): `order[p]` is the sample processed at position p.  The forward evaluates samples in
// that order (neighbouring lanes gather neighbouring table entries), the MLP backward writes the
// encoding gradient in it, and the scatter's units (one window) see long runs of equal cells on
// every level.  Keys carry the in-window index (unique keys, bitonic sort in LDS): the order is a
// deterministic function of the positions.
constexpr int SORT_W = 4096, SORT_THREADS = 1024;
__device__ __forceinline__ uint32_t sort_spread10(uint32_t v) {  // 10 bits -> every third bit
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ uint32_t sort_q10(float v, float mn, float inv) {
    const float q = (v - mn) * inv * 1024.0f;
    return (uint32_t)(int)fminf(fmaxf(q, 0.0f), 1023.0f);  // (NaN -> 0)
}
__global__ __launch_bounds__(SORT_THREADS) void sort_windows_kernel(const float* __restrict__ xyzs, int64_t n,
                                                                    const int32_t* __restrict__ n_dev, float mn,
                                                                    float inv, int32_t* __restrict__ order) {
    __shared__ unsigned long long k[SORT_W];
    if (n_dev) n = min<int64_t>(n, *n_dev);
    const int64_t base = (int64_t)blockIdx.x * SORT_W;
    if (base >= n) return;  // (uniform)
    const int cnt = (int)min<int64_t>(SORT_W, n - base);
    for (int i = threadIdx.x; i < SORT_W; i += SORT_THREADS) {
        unsigned long long key = ~0ull;  // empty slots sort last
        if (i < cnt) {
            const float* x = xyzs + 3 * (base + i);
            const uint32_t m = sort_spread10(sort_q10(x[0], mn, inv)) | (sort_spread10(sort_q10(x[1], mn, inv)) << 1) |
                               (sort_spread10(sort_q10(x[2], mn, inv)) << 2);
            key = ((unsigned long long)m << 12) | (unsigned long long)i;
        }
        k[i] = key;
    }
    __syncthreads();
    for (int size = 2; size <= SORT_W; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < SORT_W / 2; t += SORT_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;  // pair (lo, hi), lo's bit `stride` clear
                const bool up = (lo & size) == 0;
                const unsigned long long a = k[lo], b = k[hi];
                if ((a > b) == up) { k[lo] = b; k[hi] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < cnt; i += SORT_THREADS) order[base + i] = (int32_t)(base + (int64_t)(k[i] & 0xFFFull));
}

// Forward: grid-stride over 16-sample groups, one group per wave per step.
// (Round 3 measured 4 waves/SIMD at 101 us and spills at 5-6; round 5 took the register pressure
// out of the encoding instead — two levels' gathers in flight, below — and at 72 VGPRs the kernel
// runs 7 waves/SIMD: 84 us.  The waves_per_eu hint keeps the allocation in that range: without it
// the compiler's choice left 5 waves.)
// DENSITY: the grid refresh's mode 2 (encodings from encode_xcd_kernel's scratch, sigma only) as its
// own instantiation — the training forward's loop then carries no trace of it (with the scratch read
// inside the shared loop the training kernel took 136 registers, 3 waves/SIMD, and ran ~10 % slower).
template <typename T, bool DENSITY>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void field_fwd_kernel(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                        int64_t n, const int32_t* __restrict__ n_dev,
                                                        const float2* __restrict__ table, LevelTable Lt,
                                                        float xyz_min, float xyz_extent,
                                                        const typename Mfma<T>::v8* __restrict__ wpacked, int mode,
                                                        float* __restrict__ sigmas, float* __restrict__ rgbs,
                                                        typename Mfma<T>::v8* __restrict__ enc_cache,
                                                        const int32_t* __restrict__ order) {
    typedef typename Mfma<T>::v8 v8;
    __shared__ v8 Fs[N_FWD32 * 64];
    __shared__ LevelTable L;
    const int64_t n16 = (n + 15) & ~(int64_t)15;  // (mode 2, level-major scratch) per-level stride
    if (n_dev) n = min<int64_t>(n, *n_dev);  // device-resident count (static-capacity buffers)
    for (int i = threadIdx.x; i < N_FWD32 * 64; i += 256) Fs[i] = wpacked[i];
    load_levels(L, Lt);
    __syncthreads();
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    const int64_t n_groups = (n + 15) / 16;
    // (Tried: an XCD-aware renumbering (common.h xcd_block) giving each L2 whole ray patches:
    // 88 -> 109 us — the CUs of one XCD then gather the same fine-level entries at once.)
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t grp = wave0; grp < n_groups; grp += n_waves) {
        Frags<T> F;
        F.f32 = Fs + opaque_zero();  // fragments re-read from LDS every group (not hoisted)
        F.f16 = nullptr;
        const int64_t pos = grp * 16 + r;  // processing position; s = the sample it evaluates
        const bool valid = pos < n;
        const int64_t s = valid && order ? (int64_t)order[pos] : pos;
        v8 e;
        if constexpr (DENSITY) {  // the encodings of encode_xcd_kernel (mode 2: density only)
            typedef T t2 __attribute__((ext_vector_type(2)));
            const t2* el = (const t2*)enc_cache + pos;  // levels 2g, 2g+1 | 8+2g, 9+2g of sample pos
            const t2 a0 = el[(2 * g) * n16], a1 = el[(2 * g + 1) * n16];
            const t2 b0 = el[(8 + 2 * g) * n16], b1 = el[(9 + 2 * g) * n16];
            e = v8{a0[0], a0[1], a1[0], a1[1], b0[0], b0[1], b1[0], b1[1]};
        } else {
            float x = 0.f, y = 0.f, z = 0.f;
            if (valid) {
                x = (xyzs[3 * s] - xyz_min) / xyz_extent;
                y = (xyzs[3 * s + 1] - xyz_min) / xyz_extent;
                z = (xyzs[3 * s + 2] - xyz_min) / xyz_extent;
            }
            const float2 e00 = encode_level(table, L, 2 * g, x, y, z);
            const float2 e01 = encode_level(table, L, 2 * g + 1, x, y, z);
            // The last two levels' positions wait for the first two's results (an empty asm that
            // reads them), so only two levels' 16 gathers are in flight per lane, not all 32: the
            // kernel then needs 72 VGPRs instead of 120 and runs 7 waves per SIMD instead of 4 —
            // 100 -> 84 us on the bench batch (round 5, tools/field_probe.py; one level at a time:
            // 85; the pairs of an x-edge as one 16-B load: 90-98, the cache-line count does not
            // bound it; buffer loads: 90).
            asm volatile("; encode: levels 8+ after 0-7 %1 %2" : "+v"(x) : "v"(e00.x), "v"(e01.x));
            const float2 e10 = encode_level(table, L, 8 + 2 * g, x, y, z);
            const float2 e11 = encode_level(table, L, 9 + 2 * g, x, y, z);
            e = v8{(T)e00.x, (T)e00.y, (T)e01.x, (T)e01.y, (T)e10.x, (T)e10.y, (T)e11.x, (T)e11.y};
            if (enc_cache) enc_cache[grp * 64 + lane] = e;
        }
        FwdState<T> st;
        mlp_sigma<T>(F, lane, e, st);
        if (g == 0 && valid) sigmas[s] = __expf(st.h[0]);  // TruncExp forward = exp
        if (DENSITY || mode != 0) continue;
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if (valid) {
            dx = dirs[3 * s]; dy = dirs[3 * s + 1]; dz = dirs[3 * s + 2];
            const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
            dx /= nrm; dy /= nrm; dz /= nrm;
        }
        mlp_rgb<T>(F, lane, dx, dy, dz, st);
        if (g == 0 && valid) {
            rgbs[3 * s] = sigmoidf_(st.out[0]);
            rgbs[3 * s + 1] = sigmoidf_(st.out[1]);
            rgbs[3 * s + 2] = sigmoidf_(st.out[2]);
        }
    }
}

// The hash-grid encoding of the density pass (grid refresh: ~1 M points, one per hit cell, with no
// ray coherence) split by level over the XCDs: block b runs on XCD b % 8 (dispatch round-robin — a
// placement hint, nothing depends on it) and XCD x encodes levels x and 15 - x of every point, so each
// 4 MB L2 holds at most two levels' tables instead of serving all 16 (45.8 MB) from the Infinity
// Cache, and every XCD pairs a cheap coarse level with a costly fine one (round 6: x and x + 8 left
// XCDs 5-7 with levels 13-15 and the rest waiting: 225.6 -> 214.5 us for the pass on the bench grid's
// 706 K cells, profiles/round6/density_probe_pairing.log) (the sample-major forward on Morton-ordered grid points: 436 us; with every hashed level
// reading one table: 206 us — tools/field_probe.py).  Output: a level-major scratch [16][n16] of T
// pairs (172 vs 179 us for the pass with the forward's fragment-order layout, tools/density_probe.py), each level's pairs written by its own block; field_fwd_kernel mode 2
// gathers lane (g, r)'s levels {2g, 2g+1 | 8+2g, 9+2g} from it and runs sigma_net.  Same
// encode_level and operand rounding as the sample-major forward: bit-identical sigmas.
template <typename T>
__global__ __launch_bounds__(256) void encode_xcd_kernel(const float* __restrict__ xyzs, int64_t n,
                                                         const int32_t* __restrict__ n_dev,
                                                         const float2* __restrict__ table, LevelTable Lt,
                                                         float xyz_min, float xyz_extent, int nb,
                                                         T* __restrict__ enc) {
    __shared__ LevelTable L;
    load_levels(L, Lt);
    __syncthreads();
    const int64_t n16 = (n + 15) & ~(int64_t)15;  // per-level stride of the level-major scratch
    if (n_dev) n = min<int64_t>(n, *n_dev);
    const int x8 = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int l = j < nb ? x8 : 15 - x8, blk = j < nb ? j : j - nb;
    const int64_t s = (int64_t)blk * 256 + threadIdx.x;
    if (s >= n) return;
    const float x = (xyzs[3 * s] - xyz_min) / xyz_extent;
    const float y = (xyzs[3 * s + 1] - xyz_min) / xyz_extent;
    const float z = (xyzs[3 * s + 2] - xyz_min) / xyz_extent;
    const float2 a = encode_level(table, L, l, x, y, z);
    typedef T t2 __attribute__((ext_vector_type(2)));
    // level-major scratch [16][n16] of T pairs: a workgroup's 256 points of one level are one
    // contiguous 1 KB store (a fragment-order layout scattered 4-byte pieces of 64-byte records over
    // 16 workgroups on 8 XCDs: 179 vs 172 us for the pass; round 5: non-temporal point loads and
    // scratch stores, to keep the streamed data from evicting the level's table in L2 — no change)
    ((t2*)enc)[(int64_t)l * n16 + s] = t2{(T)a.x, (T)a.y};
}
}  // namespace ncn
