// Compositing, shared by forward and backward: the layout of a ray's rows, the ray segment of a
// wave, and the dispatch of long rays to whole workgroups.
#pragma once
#include "common.h"

namespace ncn {

// Compositing (volumerendering.cu:97-176 forward, :297-418 backward).  One wave per ray segment;
// the segment's samples are taken in rows of 64 consecutive samples (lane l holds sample
// row*64 + l, so every load is one contiguous 256-B piece), up to ROWS rows per round with all of
// the round's loads issued before the first use.  Per row an inclusive DPP product scan of (1 - a)
// gives the transmittance in front of each sample; the first sample whose transmittance after it
// falls to T_threshold stops the ray (it is composited but not counted, quirk q6); the row's last
// transmittance carries to the next row.  Every per-sample array is addressed through a buffer
// descriptor sized to the ray's segment (buf_rsrc): lanes past N read 0 (so a = 0, 1 - a = 1 and
// w = 0 fall out without masks) and their stores are dropped.  Per-ray values are scalar loads.

// The ray handled by this wave and its segment.  The wave index is clamped instead of returning
// early so the kernarg, rays_a and array-pointer loads issue as one scalar batch; `live` guards
// the per-ray stores of the (at most 3) surplus waves of the last block.
// Waves (rays) per workgroup of the compositors.
#ifndef CF_WPB
#define CF_WPB 4
#endif
struct RaySeg {
    int64_t ray, start;
    int N;
    bool live;
};
__device__ __forceinline__ RaySeg load_ray_seg(const int64_t* __restrict__ rays_a, int64_t R, int blk) {
    const int64_t n0 = __builtin_amdgcn_readfirstlane((int)(blk * CF_WPB + (threadIdx.x >> 6)));
    const int64_t n = n0 < R ? n0 : R - 1;
    RaySeg s;
    s.ray = rays_a[3 * n];
    s.start = rays_a[3 * n + 1];
    s.N = (int)rays_a[3 * n + 2];
    s.live = n0 < R;
    return s;
}

// Long rays (CF_LONG < N <= CF_COOP_MAX samples) are taken by a whole workgroup: wave v composites
// the ray's samples [256 v, 256 v + 256) as one 4-row block with a local carry of 1, the waves'
// segment products meet in LDS (carry-in = product of the preceding waves' products), the first
// stopping sample over the ray is the minimum of the waves' first stops, and the per-wave sums are
// added in wave order.  Every load of the ray is issued in ONE round (a single wave needs 2-4
// dependent rounds for 256 < N <= 1024, the tail that bounded the launch); 3 LDS barriers.  The
// training step's rows hold the long rays first (march_train_place), so workgroup j < n_coop takes
// row j when it is long; long rays outside the first n_coop rows (eager callers: rows in ray order)
// stay on the single-wave path.  Float order: T = carry x local prefix (vs one chained product),
// within the compositor's scan tolerance.
#define CF_LONG 256
#define CF_COOP_MAX (256 * CF_WPB)
// The n_coop workgroups at the front of the grid walk the rows b, b + n_coop, ... and stop at the
// first short one (N <= CF_LONG): with the long rays first, every long ray is taken whatever their
// number.  (Rows with N > CF_COOP_MAX are passed over and stay single-wave.)  Row `row` (long) is
// taken by a workgroup iff no row row - k * n_coop (k >= 1) is short.  Successive rows of one
// workgroup reuse its LDS without an extra barrier: every LDS array is read between the barriers
// of its own row, before the next row writes it behind a later barrier.
__device__ __forceinline__ bool cf_coop_takes(const int64_t* __restrict__ rays_a, int64_t row, int n_coop) {
    for (int64_t k = row - n_coop; k >= 0; k -= n_coop)
        if (rays_a[3 * k + 2] <= CF_LONG) return false;
    return true;
}
// How every compositor kernel opens: workgroup b < n_coop runs its workgroup path over the rows
// b, b + n_coop, ... while cf_long_row holds and is done; a wave behind them takes the ray of
// cf_own_ray, unless a workgroup already has that row (`taken`, wave-uniform).
// (One function doing both around a callable moved composite_fw_kernel<3> from 64 to 72 VGPRs.)
__device__ __forceinline__ bool cf_long_row(const int64_t* __restrict__ rays_a, int64_t R, int64_t row) {
    return row < R && (int)rays_a[3 * row + 2] > CF_LONG;
}
__device__ __forceinline__ RaySeg cf_own_ray(const int64_t* __restrict__ rays_a, int64_t R, int n_coop, bool& taken) {
    const RaySeg g = load_ray_seg(rays_a, R, (int)blockIdx.x - n_coop);
    const int64_t row = __builtin_amdgcn_readfirstlane((int)((blockIdx.x - n_coop) * CF_WPB + (threadIdx.x >> 6)));
    taken = g.N > CF_LONG && g.N <= CF_COOP_MAX && cf_coop_takes(rays_a, row, n_coop);
    return g;
}

// Alpha of ROWS rows (a, and om = 1 - a) and the inclusive product scan p of 1 - a within each row.
template <int ROWS>
__device__ __forceinline__ void cf_alpha_scan(const float (&sg)[ROWS], const float (&dl)[ROWS], float (&a)[ROWS],
                                              float (&om)[ROWS], float (&p)[ROWS]) {
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        a[r] = 1.0f - __expf(-sg[r] * dl[r]);
        om[r] = p[r] = 1.0f - a[r];
    }
    wave_incl_prod_multi<ROWS>(p);
}
// The local chain of a 4-row block: Tb = the transmittance in front of each sample with 1 in front
// of the block; returns the block's product.  A long ray's transmittance is carry x Tb on the
// single-wave path and on the workgroup path alike: the same float operations in the same order.
__device__ __forceinline__ float cf_local_chain(const float (&p)[4], const float (&om)[4], float (&Tb)[4]) {
    float Tc = 1.0f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        Tb[r] = Tc * wave_shr1_dpp(p[r], 1.0f);
        Tc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Tb[r] * om[r]), 63));
    }
    return Tc;
}

}  // namespace ncn
