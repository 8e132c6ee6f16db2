// Marcher stage 2: the wave-parallel walk of one ray at constant dt, its eager kernel and the first
// launch of the training step's fused marcher (AABB test + jitter + walk).
#pragma once
#include "vren_aabb.h"
#include "vren_march.h"

namespace ncn {

// raymarching_train pass 1, wave-parallel form (exp_step_factor == 0, i.e. constant dt; the
// reference's configs at scale 0.5).  Both branches of the reference walk advance t along the same
// chain c_{k+1} = fl(c_k + dt): an occupied probe emits and does `t += dt`, an empty one does
// `do t += dt; while (t < t_target)` (raymarching.cu:221-233).  So the walk visits a subsequence of
// that chain: after an occupied position k comes k+1, after an empty one the first j > k with
// c_j >= t_target(k).  One wave takes one ray, 64*P chain positions per iteration (lane l holds
// positions l + 64 j): the chain values come in closed form (march_chain), every position is
// probed at once (one bitfield gather per lane instead of one serial walk step), and a short
// scalar loop over ballot masks resolves which positions the walk visits.  Emitted samples are
// compacted (mbcnt) into the slab row.  Bit-identical to the serial walk: same fmaf positions,
// same probe, same target expression, same chain values.

// Chain values in closed form.  Inside one binade [2^e, 2^(e+1)) with ulp u, c + dt rounds to
// c + u*round(dt/u) when dt/u is not a tie, i.e. a constant step in the bit pattern; with a tie
// (dt/u = m + 1/2, possible in at most one binade) round-to-even makes every result even, so the
// step is constant from the second step on.  The two first steps are real float adds (r1, r) and
// the rest of the binade is bits(v) + r1 + (k-1) r, valid while the exponent field is unchanged
// (then the exact sum is below 2^(e+1), so the in-binade rounding applies); the step that leaves
// the binade is again a real float add.  Fills c[j] = c_{lane + 64 j} for the window starting at
// cb (index 0) and returns c_{64P}.  A chain that stops advancing (dt < u/2: the reference would
// spin forever) is frozen and the caller's window cap ends the ray.
template <int P>
__device__ __forceinline__ float march_chain(float cb, float dt, int lane, float (&c)[P]) {
    constexpr int L = 64 * P;
#pragma unroll
    for (int j = 0; j < P; j++) c[j] = cb;
    int j0 = 0;
    float v = cb;
    for (;;) {
        const uint32_t bv = __float_as_uint(v);
        const float v1 = v + dt;
        const uint32_t b1 = __float_as_uint(v1);
        uint32_t r1 = b1 - bv, r = 0;
        int K;
        float vn;
        if ((bv >> 23) != (b1 >> 23) || bv == 0u) {
            K = 0;
            vn = v1;
        } else {
            const float v2 = v1 + dt;
            const uint32_t b2 = __float_as_uint(v2);
            if ((b2 >> 23) != (b1 >> 23)) {
                K = 1;
                vn = v2;
            } else {
                r = b2 - b1;
                if (r == 0u) {  // frozen chain (reference: endless loop)
#pragma unroll
                    for (int j = 0; j < P; j++)
                        if (lane + 64 * j > j0) c[j] = v;
                    return v;
                }
                const uint32_t room = (bv | 0x7FFFFFu) - bv - r1;  // bits left in the binade after step 1
                // steps in the binade: room / r + 1 (the division only when the binade ends in the window)
                K = (uint64_t)room >= (uint64_t)(L - 1) * r ? L : (int)(room / r + 1u);
                vn = __uint_as_float(bv + r1 + (uint32_t)(K - 1) * r) + dt;
            }
        }
#pragma unroll
        for (int j = 0; j < P; j++) {
            const int i = lane + 64 * j;
            if (i > j0 && i <= j0 + K) c[j] = __uint_as_float(bv + r1 + (uint32_t)(i - j0 - 1) * r);
        }
        if (j0 + K >= L) return __uint_as_float(bv + r1 + (uint32_t)(L - j0 - 1) * r);
        const int J = j0 + K + 1;
        if (J == L) return vn;
#pragma unroll
        for (int j = 0; j < P; j++)
            if (lane + 64 * j == J) c[j] = vn;
        j0 = J;
        v = vn;
    }
}

// c[] as seen from lane `idx` (idx in [0, 63])
__device__ __forceinline__ float lane_f(float v, int idx) { return __int_as_float(__builtin_amdgcn_ds_bpermute(idx << 2, __float_as_int(v))); }
__device__ __forceinline__ int lane_i(int v, int idx) { return __builtin_amdgcn_ds_bpermute(idx << 2, v); }

// First lane j > lane whose chain value reaches T (64 if none): the position an empty probe's skip
// lands on (do t += dt while t < T).  The chain steps are dt up to rounding (< ulp/2 each), so
// lane + ceil((T - c)/dt) is within one of the answer; one check either side fixes it, and a wave
// whose estimate still fails (only for steps far off dt) falls back to a binary search.
__device__ __forceinline__ int march_skip_lane(float c, float T, float dt, int lane) {
    const float q = ceilf((T - c) / dt);
    int j = lane + (int)fminf(fmaxf(q, 1.0f), 65.0f);
    if (j > 64) j = 64;
    const float cm = lane_f(c, min(j - 1, 63));  // c at j - 1 (>= lane)
    const float cj = lane_f(c, min(j, 63));
    if (j - 1 > lane && cm >= T) j -= 1;
    else if (j < 64 && cj < T) j += 1;
    const float cm2 = lane_f(c, min(j - 1, 63));
    const float cj2 = lane_f(c, min(j, 63));
    const bool ok = (j - 1 == lane || cm2 < T) && (j == 64 || cj2 >= T);
    if (__ballot(!ok)) {  // binary search: last position p >= lane with c_p < T, answer p + 1
        int p = lane;
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1) {
            const int qn = p + st;
            const float cq = lane_f(c, min(qn, 63));
            if (qn <= 63 && cq < T) p = qn;
        }
        j = p + 1;
    }
    return j;
}

// Positions the walk visits in this sub-window, starting at lane s (uniform), given every lane's
// successor nxt (> lane; 64 = beyond): binary lifting over nxt (jump tables of 1, 2, 4 .. 32 steps),
// then every lane walks the largest jumps from s that do not pass it and checks where it lands.
__device__ __forceinline__ uint64_t march_visited(int nxt, int s, int lane) {
    int J[6];
    J[0] = nxt;
#pragma unroll
    for (int i = 1; i < 6; i++) {
        const int v = lane_i(J[i - 1], min(J[i - 1], 63));
        J[i] = J[i - 1] >= 64 ? 64 : v;
    }
    int cur = s;
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        const int v = lane_i(J[i], min(cur, 63));
        const int cand = cur >= 64 ? 64 : v;
        if (cand <= lane) cur = cand;
    }
    return __ballot(cur == lane && lane >= s);
}

// The wave-parallel walk of one ray (raymarching.cu:195-279 with constant dt): samples to the
// ray's slab row (sx/st/sd), returns their count (wave-uniform).
template <bool ONE_CASCADE, int P>
__device__ __forceinline__ int march_walk_wave(const MarchConst& m, const uint8_t* __restrict__ bitfield, float ox,
                                               float oy, float oz, float dx, float dy, float dz, float t1, float t2,
                                               float noise_r, float dt, int lane, float* __restrict__ sx,
                                               float* __restrict__ st, float* __restrict__ sd) {
    const float dxi = 1.0f / dx, dyi = 1.0f / dy, dzi = 1.0f / dz;
    int n = 0;
    if (t1 >= 0) {  // :195-198; a miss (t1 = -1) never enters the loop (:204)
        t1 = fmaf(dt, noise_r, t1);
        float cb = t1;
        bool pend = false, done = false;
        float ptgt = 0.f;
        int s = 0;  // next visited lane of the current sub-window (when !pend)
        for (int it = 0; it < (1 << 16) && !done; it++) {
            float c[P];
            const float cnext = march_chain<P>(cb, dt, lane, c);
            float X[P], Y[P], Z[P], tgt[P];
            bool occ[P];
#pragma unroll
            for (int j = 0; j < P; j++) {
                X[j] = fmaf(c[j], dx, ox);
                Y[j] = fmaf(c[j], dy, oy);
                Z[j] = fmaf(c[j], dz, oz);
                int nx, ny, nz;
                float mip_bound;
                uint32_t cbi = 0xFFFFFFFFu, cbv = 0;
                occ[j] = probe<ONE_CASCADE>(m, bitfield, X[j], Y[j], Z[j], dt, nx, ny, nz, mip_bound, cbi, cbv);
                // where an empty probe at this position would skip to
                tgt[j] = skip_target(m, c[j], X[j], Y[j], Z[j], dx, dy, dz, dxi, dyi, dzi, nx, ny, nz, mip_bound);
            }
#pragma unroll
            for (int j = 0; j < P; j++) {
                if (done) break;
                const uint64_t lt_m = __ballot(c[j] < t2);  // loop condition t < t2 (:204)
                const uint64_t occ_m = __ballot(occ[j]);
                if (pend) {
                    const uint64_t mm = __ballot(c[j] >= ptgt);
                    if (!mm) continue;  // the skip runs past this sub-window
                    s = __builtin_ctzll(mm);
                    pend = false;
                }
                // successor of every position if the walk visits it (64 = beyond this sub-window)
                // (march_skip_lane reads other lanes: evaluated by the whole wave, then selected)
                const int skip = march_skip_lane(c[j], tgt[j], dt, lane);
                const int nxt = !(c[j] < t2) ? 64 : (occ[j] ? lane + 1 : skip);  // 64: the walk ends here
                const uint64_t vis = march_visited(nxt, s, lane);
                const uint64_t term = vis & ~lt_m;
                uint64_t emit = vis & occ_m & lt_m;
                const int room = m.max_samples - n;
                if (__popcll(emit) >= room) {  // the room-th sample ends the walk (:204 n < m.max_samples)
                    uint64_t e2 = emit;
                    for (int q = 1; q < room; q++) e2 &= e2 - 1;
                    const int last = __builtin_ctzll(e2);
                    emit &= (last == 63) ? ~0ull : ((2ull << last) - 1);
                    done = true;
                }
                if (term) {
                    emit &= (1ull << __builtin_ctzll(term)) - 1;
                    done = true;
                }
                if (emit) {
                    if ((emit >> lane) & 1) {
                        const int k = n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(emit >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((uint32_t)emit, 0));
                        sx[3 * k] = X[j];
                        sx[3 * k + 1] = Y[j];
                        sx[3 * k + 2] = Z[j];
                        st[k] = c[j];
                        sd[k] = dt;
                    }
                    n += __popcll(emit);
                }
                if (!done) {  // carry: after the last visited position
                    const int lastv = 63 - __builtin_clzll(vis);
                    if ((occ_m >> lastv) & 1) {
                        s = 0;  // emitted at lane lastv (== 63): the next position is lane 0 of the next sub-window
                    } else {
                        pend = true;  // an empty position whose skip target lies past this sub-window
                        ptgt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tgt[j]), lastv));
                    }
                }
            }
            cb = cnext;
        }
    }
    return n;
}

template <bool ONE_CASCADE, int P>
__global__ __launch_bounds__(256) void march_train_wave_kernel(
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ hits_t,
    const float* __restrict__ noise, int64_t R, const uint8_t* __restrict__ bitfield, int cascades, float scale,
    int G, int max_samples, int32_t* __restrict__ counts, float* __restrict__ slab_xyz,
    float* __restrict__ slab_t, float* __restrict__ slab_dt) {
    const int lane = threadIdx.x & 63;
    const int64_t r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (r >= R) return;
    const MarchConst m = make_march_const(cascades, scale, 0.0f, G, max_samples, scale);
    const float t1 = hits_t[2 * r];
    const int n = march_walk_wave<ONE_CASCADE, P>(
        m, bitfield, rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2], rays_d[3 * r], rays_d[3 * r + 1],
        rays_d[3 * r + 2], t1, hits_t[2 * r + 1], t1 >= 0 ? noise[r] : 0.f, calc_dt(m, 0.0f), lane,
        slab_xyz + r * (int64_t)max_samples * 3, slab_t + r * (int64_t)max_samples, slab_dt + r * (int64_t)max_samples);
    if (lane == 0) counts[r] = n;
}

// ---------------------------------------------------------------------------------------------
// raymarching_train for the training step in TWO launches (constant dt), replacing ray_aabb +
// rand + walk + scan + pack:
//  1. march_train_walk2: per ray (one wave) the single-AABB intersection with render()'s near
//     clamp (intersection.cu:5-56 at max_hits 1, rendering.py:28; slab_test, as
//     ray_aabb_kernel<1>), the jitter (custom_functions.py:83: torch.rand_like; here `noise` or, when
//     NULL, a counter-based uniform of (seed, *rng_ctr, ray)), the walk into the ray's slab row;
//     counts per ray and the sum of each workgroup's 4 rays;
//  2. march_train_place: every workgroup sums the sums of the workgroups before it (all loads in
//     one round trip, no inter-workgroup waiting), places its 4 rays (rays_a) and copies their slab
//     rows into the packed outputs; the last workgroup writes counter = {S, R}.
// (A single-pass decoupled look-back version was slower: the look-back of late workgroups walks
// back through many not-yet-prefixed predecessors, one memory round trip per 64 of them.)
__device__ __forceinline__ float march_uniform(uint64_t seed, uint64_t ctr, uint32_t r) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (ctr * 0x100000001B3ull + r + 1u);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(uint32_t)(z >> 40) * (1.0f / 16777216.0f);
}

constexpr int PLACE_MAX_WG = 256 * 16;  // workgroup sums one place workgroup can add in one round trip
// rays_a ROW order of the training step: rays with more than PLACE_LONG samples (more than one
// round of the compositors' row blocks) take the first rows, so the compositors dispatch their
// waves first and their extra round trip overlaps the rest of the launch.  Sample segments stay in
// ray order.  (The reference's rows and starts are both in atomicAdd order, raymarching.cu:237-241:
// any row order is within its contract; consumers index outputs by rays_a[:, 0].)
constexpr int PLACE_LONG = 256;

template <bool ONE_CASCADE, int P>
__global__ __launch_bounds__(256) void march_train_walk2_kernel(
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t R, float cx, float cy, float cz,
    float hx, float hy, float hz, float near_distance, const float* __restrict__ noise, uint64_t seed,
    const int64_t* __restrict__ rng_ctr, const uint8_t* __restrict__ bitfield, int cascades, float scale, int G,
    int max_samples, float* __restrict__ slab_xyz, float* __restrict__ slab_t, float* __restrict__ slab_dt,
    int32_t* __restrict__ counts, int32_t* __restrict__ wg_sum) {
    __shared__ int cnt_s[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + wv));
    const bool live = r0 < R;
    const int64_t r = live ? r0 : R - 1;
    const MarchConst m = make_march_const(cascades, scale, 0.0f, G, max_samples, scale);
    const float o[3] = {rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2]};
    const float d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
    const float c3[3] = {cx, cy, cz}, h3[3] = {hx, hy, hz};
    const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
    float t1, t2;
    slab_test(o, inv, c3, h3, t1, t2);
    if (t2 > 0) t1 = fmaxf(t1, 0.0f);
    else { t1 = -1.0f; t2 = -1.0f; }
    if (t1 >= 0.0f && t1 < near_distance) t1 = near_distance;
    float nz = 0.f;
    if (t1 >= 0) nz = noise ? noise[r] : march_uniform(seed, rng_ctr ? (uint64_t)*rng_ctr : 0ull, (uint32_t)r);
    int n = 0;
    if (live)
        n = march_walk_wave<ONE_CASCADE, P>(m, bitfield, o[0], o[1], o[2], d[0], d[1], d[2], t1, t2, nz,
                                            calc_dt(m, 0.0f), lane, slab_xyz + r * (int64_t)max_samples * 3,
                                            slab_t + r * (int64_t)max_samples, slab_dt + r * (int64_t)max_samples);
    if (lane == 0) {
        cnt_s[wv] = n;
        if (live) counts[r] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // sample sum | number of long rays << 26 (rays placed first by march_train_place)
        int nl = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) nl += cnt_s[w] > PLACE_LONG;
        wg_sum[blockIdx.x] = (cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3]) | (nl << 26);
    }
}

}  // namespace ncn
