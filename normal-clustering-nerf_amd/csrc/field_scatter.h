#pragma once
#include "field_grid.h"
#include "field_bwd_mlp.h"  // (with field_de_ws.h, field_diag.h)

namespace ncn {
// Scatter of the encoding gradient into the fp32 table gradient (tcnn kernel_grid_backward).
// Hash-grid gradients are extremely local: the samples of one ray stay in the same cell of a
// coarse level for tens of steps, and the rays of a patch re-touch the same entries (per
// 2-8K-sample span the contributions per distinct entry are ~460 at level 0 and still ~6 at
// level 15).  So the work is organised around runs and a per-workgroup LDS table:
//  * a unit of work is (span of consecutive samples, level): 1024 lanes x C samples x rounds;
//  * a lane sums the eight corner contributions of its consecutive samples in the same cell in
//    registers (a run) and hands a finished run to the table;
//  * the lanes' samples are read from a copy of the positions in the unit's load order (sc_perm,
//    written by the MLP pass): a wave's round reads one contiguous stretch (round 6: 192 -> 176 us,
//    the coarse units' strided loads had cost one cache line per lane per load);
//  * coarse levels [0, SC_CELL_HI) are CELL-keyed: finished runs are queued per wave and added by
//    full-wave passes (sc_drain_cells): one lookup of the run's cell in a 4-way set-associative LDS
//    table and 16 ds_add_u64 into the cell's corner-major sums; fine
//    levels are ENTRY-keyed (sc_add): each of the 8 corners looked up in its own 4-way set (one
//    ds_read_b128 per set, ds_cmpst to claim a way) and its (x, y) added with two ds_add_u64;
//  * sums are 64-bit FIXED-POINT (exact integer arithmetic: order-independent and reproducible; an
//    LDS f32 atomic costs ~3 cycles per active lane on gfx950 against ~13 per wave-instruction for a
//    u64 add, and f32 slot sums measured 2-3x slower under the same-slot conflicts).  The
//    scale of a level is 2^k, k = 60 - log2(unit samples) - e (fine units 46 - e), max|dE| < 2^e (the
//    MLP pass records max|dE| per level), so an entry's unit sum stays below 2^62 and every addend
//    below 2^51 (sc_fix).  A corner whose set is full goes
//    straight to a global f32 atomic;
//  * at the end of the unit the claimed slots (the `used` list) are flushed with one f32 global
//    atomic per non-zero sum and reset.  A unit whose gradient is not finite adds every run straight
//    to global memory (NaN/Inf propagate as in the f32 path).
constexpr int SC_WAYS = 4;       // 4-way set associative: one ds_read_b128 per lookup
constexpr int SC_SLOT_BYTES = 4 + 8 + 8 + 2;  // key, x and y sums, `used` entry
constexpr int SC_SETS_DIR = 1536;  // entry-keyed layout: 6 144 slots (132 KB)
// Cell-keyed layout (the coarse levels [0, SC_CELL_HI)): a slot is one grid CELL of the level and
// holds the 64-bit sums of its 8 corners' x and y (corner-major: vals[(2c + xy) * slots + slot]).
constexpr int SC_CELL_VALS = 16;
// Finished coarse runs are queued per wave (key + 16 f32 sums, 68 B) and added to the table by a
// full-wave pass once the queue would overflow (sc_push_run / sc_drain_cells): a coarse sample step
// ends a run in only ~6-30 of 64 lanes, and adding them at once cost a set read and 16 ds_add_u64
// wave-instructions (plus 16 fixed-point conversions) per step for those few lanes.
// (Round 6: queued 180 vs 189 us for the whole scatter, levels 0-5 alone 43 vs 62 us per unit,
// profiles/round6/scatter_probe_queue.log; the table shrank from 1 024 cell slots for the queues.)
constexpr int SC_SETS_CELL = 160;  // 640 cell slots (86 KB) beside the run queues (70 KB)
constexpr int SC_QUEUE = 64;       // runs per wave queue
constexpr int SC_CELL_TABLE_BYTES = SC_SETS_CELL * SC_WAYS * (4 + SC_CELL_VALS * 8 + 2);
constexpr int SC_QUEUE_BYTES = SC_WAVES * SC_QUEUE * (4 + SC_CELL_VALS * 4);
constexpr int sc_max(int a, int b) { return a > b ? a : b; }
constexpr int SC_ARENA = sc_max(SC_CELL_TABLE_BYTES + SC_QUEUE_BYTES, SC_SETS_DIR * SC_WAYS * SC_SLOT_BYTES);
static_assert(SC_CELL_TABLE_BYTES % 16 == 0, "run queues 16-B aligned");
constexpr uint32_t SC_EMPTY = 0xFFFFFFFFu;
constexpr int SC_BATCH = 2;  // corners per batch of set reads in sc_add (2: 232 us, 4: 238 us (spills), 8: 298 us;
                             // round 5: 4 at 124 VGPRs 196 us (4 spills); at 120, no spills: 194-195 vs 190)

__device__ __forceinline__ uint32_t sc_set(uint32_t e, uint32_t sets) { return __umulhi(e * 0x9E3779B1u, sets); }

// round(v * 2^k) as int64 (|v * 2^k| < 2^51): v * 2^k is exact in f64, adding 1.5 * 2^52 rounds it
// to an integer in the low mantissa bits (round-to-nearest-even), and the bit pattern minus that of
// 1.5 * 2^52 is the two's-complement integer.  Three f64/int ops instead of an f32 hi/lo split.
__device__ __forceinline__ long long sc_fix(float v, int k) {
    const double magic = 6755399441055744.0;  // 1.5 * 2^52
    const double y = fma((double)v, __longlong_as_double((long long)(1023 + k) << 52), magic);
    return __double_as_longlong(y) - __double_as_longlong(magic);
}

// The current layout's arrays inside the arena (uniform pointers) and the per-workgroup counters.
struct ScShared {
    uint32_t* keys;
    long long *valx, *valy;  // (cell layout: valx = the 16 corner-major arrays)
    uint16_t* used;          // slots claimed since the last flush, in claim order
    float4* qval;            // (cell layout) the waves' run queues: [wave][SC_QUEUE][4] float4 (16 sums)
    uint32_t* qkey;          //               and their cell keys [wave][SC_QUEUE]
    uint32_t sets;
    int slots;
    int* fill;
    int* grab;  // the unit's grab counter (fine levels)
};
enum { SC_MODE_DIR = 0, SC_MODE_CELL = 1 };
__device__ __forceinline__ ScShared sc_layout(char* arena, int* fill, int mode) {
    ScShared sh;
    sh.sets = mode == SC_MODE_CELL ? SC_SETS_CELL : SC_SETS_DIR;
    sh.slots = (int)sh.sets * SC_WAYS;
    sh.valx = (long long*)arena;  // 8-B arrays first, then keys, used
    sh.valy = mode == SC_MODE_CELL ? sh.valx + (SC_CELL_VALS - 1) * sh.slots : sh.valx + sh.slots;
    sh.keys = (uint32_t*)(sh.valy + sh.slots);
    sh.used = (uint16_t*)(sh.keys + sh.slots);
    sh.qval = (float4*)(arena + SC_CELL_TABLE_BYTES);
    sh.qkey = (uint32_t*)(sh.qval + SC_WAVES * SC_QUEUE * 4);
    sh.fill = fill;
    return sh;
}

// Level geometry of the unit, uniform.
struct ScLevel {
    float scale;
    uint32_t res, params, off;
    bool dense, direct;
    int k;
};

__device__ __forceinline__ void sc_corner_entries(const ScLevel& L, uint32_t px, uint32_t py, uint32_t pz,
                                                  uint32_t (&e)[8]) {
    if (L.dense) {
        const uint32_t b0 = px + L.res * py + L.res * L.res * pz;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            e[c] = b0 + (c & 1) + ((c >> 1) & 1) * L.res + ((c >> 2) & 1) * L.res * L.res;
            e[c] = e[c] < L.params ? e[c] : e[c] % L.params;  // as grid_index (boundary corner)
        }
    } else {  // params is 2^19 on every hashed level
        const uint32_t hy0 = py * 2654435761u, hy1 = (py + 1) * 2654435761u;
        const uint32_t hz0 = pz * 805459861u, hz1 = (pz + 1) * 805459861u;
#pragma unroll
        for (int c = 0; c < 8; c++)
            e[c] = ((px + (c & 1)) ^ ((c & 2) ? hy1 : hy0) ^ ((c & 4) ? hz1 : hz0)) & (L.params - 1);
    }
}

// Entry-keyed table: one contribution set per lane (cell px,py,pz; v = the 8 corners' (x, y) sums).
// Called by the whole wave; lanes with all-zero v add nothing.
__device__ __forceinline__ void sc_add(ScShared& sh, int lane, uint32_t px, uint32_t py, uint32_t pz,
                                       const float (&v)[16], const ScLevel& L, float* __restrict__ grad) {
    uint32_t e[8];
    sc_corner_entries(L, px, py, pz, e);
    if (L.direct) {
#pragma unroll
        for (int c = 0; c < 8; c++) {
            if (v[2 * c] != 0.f || v[2 * c + 1] != 0.f) {
                atomicAdd(grad + 2 * (size_t)(L.off + e[c]), v[2 * c]);
                atomicAdd(grad + 2 * (size_t)(L.off + e[c]) + 1, v[2 * c + 1]);
            }
        }
        return;
    }
    // Corners in batches of SC_BATCH: the batch's set reads (ds_read_b128) are issued together and
    // waited for once, then the hits and claims are resolved, then the batch's fixed-point adds
    // (ds_add_u64, no return) are issued back to back — a few LDS round trips per record instead of
    // two per corner.  A miss claims the first empty way of its set with ds_cmpst (a uniform branch
    // skips the claim step when no lane of the wave misses); a lost claim re-reads the set once;
    // a full set falls back to a global atomic.  Zero corners (beyond the span / zero dE / a lane
    // with no finished run) take part with nothing to add.
    uint32_t newmask = 0;
    int slot[8];
#pragma unroll
    for (int c0 = 0; c0 < 8; c0 += SC_BATCH) {
        uint4 kk[SC_BATCH];
        int p0[SC_BATCH];
#pragma unroll
        for (int b = 0; b < SC_BATCH; b++) {
            p0[b] = SC_WAYS * sc_set(e[c0 + b], sh.sets);
            kk[b] = *(const uint4*)&sh.keys[p0[b]];
        }
        int sl[SC_BATCH];
        bool vc[SC_BATCH], miss = false;
#pragma unroll
        for (int b = 0; b < SC_BATCH; b++) {
            const uint32_t k = e[c0 + b];
            vc[b] = (v[2 * (c0 + b)] != 0.f) | (v[2 * (c0 + b) + 1] != 0.f);
            sl[b] = kk[b].x == k ? p0[b] : kk[b].y == k ? p0[b] + 1 : kk[b].z == k ? p0[b] + 2
                  : kk[b].w == k ? p0[b] + 3 : -1;
            miss |= vc[b] && sl[b] < 0;
        }
        if (__ballot(miss)) {  // uniform
#pragma unroll
            for (int b = 0; b < SC_BATCH; b++) {
                if (vc[b] && sl[b] < 0) {
                    const uint32_t k = e[c0 + b];
#pragma unroll
                    for (int attempt = 0; attempt < 2 && sl[b] < 0; attempt++) {
                        if (attempt) {  // lost a claim: look again
                            asm volatile("" ::: "memory");
                            kk[b] = *(const uint4*)&sh.keys[p0[b]];
                        }
                        sl[b] = kk[b].x == k ? p0[b] : kk[b].y == k ? p0[b] + 1 : kk[b].z == k ? p0[b] + 2
                              : kk[b].w == k ? p0[b] + 3 : -1;
                        if (sl[b] >= 0) break;
                        const int cl = kk[b].x == SC_EMPTY ? p0[b] : kk[b].y == SC_EMPTY ? p0[b] + 1
                                     : kk[b].z == SC_EMPTY ? p0[b] + 2 : kk[b].w == SC_EMPTY ? p0[b] + 3 : -1;
                        if (cl < 0) break;  // set full
                        const uint32_t got = atomicCAS(&sh.keys[cl], SC_EMPTY, k);
                        if (got == SC_EMPTY) { sl[b] = cl; newmask |= 1u << (c0 + b); }
                        else if (got == k) sl[b] = cl;
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < SC_BATCH; b++) {
            const int c = c0 + b;
            slot[c] = sl[b];
            if (vc[b] && sl[b] >= 0) {
                atomicAdd((unsigned long long*)&sh.valx[sl[b]], (unsigned long long)sc_fix(v[2 * c], L.k));
                atomicAdd((unsigned long long*)&sh.valy[sl[b]], (unsigned long long)sc_fix(v[2 * c + 1], L.k));
            }
        }
        bool full = false;
#pragma unroll
        for (int b = 0; b < SC_BATCH; b++) full |= vc[b] && sl[b] < 0;
        if (__ballot(full)) {  // uniform: some lane's set is full of other entries
#pragma unroll
            for (int b = 0; b < SC_BATCH; b++) {
                const int c = c0 + b;
                if (vc[b] && sl[b] < 0) {
                    if (v[2 * c] != 0.f) atomicAdd(grad + 2 * (size_t)(L.off + e[c]), v[2 * c]);
                    if (v[2 * c + 1] != 0.f) atomicAdd(grad + 2 * (size_t)(L.off + e[c]) + 1, v[2 * c + 1]);
                }
            }
        }
    }
    // append the claimed slots to `used`: one LDS atomic per wave
    const int mine = __builtin_popcount(newmask);
    const float incl = wave_incl_sum_dpp((float)mine);
    const int wtot = (int)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63));
    if (wtot) {
        int base = 0;
        if (lane == 0) base = atomicAdd(sh.fill, wtot);
        base = __builtin_amdgcn_readfirstlane(base);
        int pos = base + (int)incl - mine;
#pragma unroll
        for (int c = 0; c < 8; c++)
            if (newmask & (1u << c)) sh.used[pos++] = (uint16_t)slot[c];
    }
}

// Sample position in [0,1]^3 as the forward computes it ((x - min) / extent; a power-of-two
// extent — 1.0 at the configs' scale 0.5 — multiplies by its exact reciprocal instead).
struct ScNorm {
    float mn, ext, inv;
    bool pow2;
    __device__ __forceinline__ float operator()(float v) const { return pow2 ? (v - mn) * inv : (v - mn) / ext; }
};

// The encoding gradient as the MLP pass stored it (field_bwd_kernel): pairs of the operand type, fp16
// at the chain's loss scale or bf16 unscaled; decoded to f32 and unscaled (1/S: a power of two, exact).
struct ScDE {
    float inv;
    bool bf16;
    __device__ __forceinline__ float2 operator()(uint32_t w) const {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 h = __builtin_bit_cast(h2, w);
        const float x = bf16 ? __uint_as_float(w << 16) : (float)h[0];
        const float y = bf16 ? __uint_as_float(w & 0xFFFF0000u) : (float)h[1];
        return make_float2(x * inv, y * inv);
    }
};

__device__ __forceinline__ void sc_corner_sums(const LevelPos& p, float2 g, float (&v)[16]) {
    // corner weights in the forward's association ((wx * wy) * wz)
    const float wx[2] = {1.0f - p.fx, p.fx}, wy[2] = {1.0f - p.fy, p.fy}, wz[2] = {1.0f - p.fz, p.fz};
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const float w = (wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2];
        v[2 * c] = fmaf(w, g.x, v[2 * c]);
        v[2 * c + 1] = fmaf(w, g.y, v[2 * c + 1]);
    }
}

// A lane's C consecutive samples (normalised positions and dE of the unit's level), loaded at the
// start of the unit in one batch; samples past the end carry dE = 0.
template <int C>
struct ScChunk {
    float x[C], y[C], z[C];
    float2 g[C];
};
// C is 2 or 4 and the lane's first sample sb a multiple of C: the chunk's xyz (12C bytes) and dE
// (4C bytes) are 16-B (C = 4) / 8-B (C = 2) aligned pieces, loaded with dwordx4 / dwordx2 — a lane
// reads contiguous bytes, so fewer, wider load instructions (the lane-strided pattern costs TA
// cycles per touched cache line).  A partial last chunk falls back to per-sample loads.
template <int C>
__device__ __forceinline__ void sc_load_de(ScChunk<C>& ch, const uint32_t* __restrict__ p, const ScDE& de) {
    if constexpr (C == 4) {
        const uint4 v = *(const uint4*)p;
        ch.g[0] = de(v.x); ch.g[1] = de(v.y); ch.g[2] = de(v.z); ch.g[3] = de(v.w);
    } else {
        const uint2 v = *(const uint2*)p;
        ch.g[0] = de(v.x); ch.g[1] = de(v.y);
    }
}
// xyzs: the unit class's permuted positions (sc_perm) with pb = the chunk's place in them, or (with
// `order`, pb unused) the sample-ordered positions gathered through order.
template <int C>
__device__ __forceinline__ void sc_load_chunk(ScChunk<C>& ch, int64_t sb, int64_t pb, int64_t s1,
                                               const float* __restrict__ xyzs, const uint32_t* __restrict__ dEl,
                                               const ScDE& de, const ScNorm& nrm, const int32_t* __restrict__ order) {
    static_assert(C == 2 || C == 4, "chunk of 2 or 4 samples");
    float xs[3 * C];
    if (order) {  // positions sb.. in processing order: dE contiguous, positions gathered
        int64_t src[C];
#pragma unroll
        for (int i = 0; i < C; i++) src[i] = sb + i < s1 ? (int64_t)order[sb + i] : -1;
        if (sb + C <= s1) {
            sc_load_de<C>(ch, dEl + sb, de);
        } else {
#pragma unroll
            for (int i = 0; i < C; i++) ch.g[i] = src[i] >= 0 ? de(dEl[sb + i]) : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < C; i++) {
            const int64_t sc = src[i] >= 0 ? src[i] : 0;
            xs[3 * i] = xyzs[3 * sc];
            xs[3 * i + 1] = xyzs[3 * sc + 1];
            xs[3 * i + 2] = xyzs[3 * sc + 2];
        }
    } else if (sb + C <= s1) {
        if constexpr (C == 4) {
            const float4* px = (const float4*)(xyzs + 3 * pb);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const float4 v = px[q];
                xs[4 * q] = v.x; xs[4 * q + 1] = v.y; xs[4 * q + 2] = v.z; xs[4 * q + 3] = v.w;
            }
        } else {
            const float2* px = (const float2*)(xyzs + 3 * pb);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const float2 v = px[q];
                xs[2 * q] = v.x; xs[2 * q + 1] = v.y;
            }
        }
        sc_load_de<C>(ch, dEl + sb, de);
    } else {
#pragma unroll
        for (int i = 0; i < C; i++) {
            const bool in = sb + i < s1;
            const int64_t sc = in ? sb + i : 0, pc = in ? pb + i : 0;
            ch.g[i] = in ? de(dEl[sc]) : make_float2(0.f, 0.f);
            xs[3 * i] = in ? xyzs[3 * pc] : 0.f;
            xs[3 * i + 1] = in ? xyzs[3 * pc + 1] : 0.f;
            xs[3 * i + 2] = in ? xyzs[3 * pc + 2] : 0.f;
        }
    }
#pragma unroll
    for (int i = 0; i < C; i++) {
        ch.x[i] = nrm(xs[3 * i]);
        ch.y[i] = nrm(xs[3 * i + 1]);
        ch.z[i] = nrm(xs[3 * i + 2]);
    }
}

// Fine levels: the lane's consecutive samples in the same cell are summed in registers (a run), and
// a run's 8 corners go to the table when the cell changes (sc_add is called by the whole wave;
// lanes without a finished run take part with zeros).
template <int C>
__device__ __forceinline__ void sc_direct(ScShared& sh, int lane, const ScChunk<C>& ch, const ScLevel& L,
                                          float* __restrict__ grad) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = 0.f;
    LevelPos p = level_pos(L.scale, ch.x[0], ch.y[0], ch.z[0]);
    sc_corner_sums(p, ch.g[0], v);
#pragma unroll
    for (int i = 1; i <= C; i++) {
        LevelPos q = p;
        bool emit = true;
        if (i < C) {
            q = level_pos(L.scale, ch.x[i], ch.y[i], ch.z[i]);
            emit = q.px != p.px || q.py != p.py || q.pz != p.pz;
        }
        if (__ballot(emit)) {  // uniform
            float ve[16];
#pragma unroll
            for (int j = 0; j < 16; j++) ve[j] = emit ? v[j] : 0.f;
            sc_add(sh, lane, p.px, p.py, p.pz, ve, L, grad);
        }
        if (i < C) {
#pragma unroll
            for (int j = 0; j < 16; j++) v[j] = emit ? 0.f : v[j];
            sc_corner_sums(q, ch.g[i], v);
        }
        p = q;
    }
}

// ---- cell-keyed form (coarse levels) ----
// One LDS lookup per run instead of one per corner: the run's cell (px, py, pz) is the key
// (px | py << 11 | pz << 22; cells outside that range go straight to global memory) and its 8
// corners' sums are 16 ds_add_u64 into the slot's corner arrays.  The flush forms each claimed
// cell's corner entries and adds them to the table gradient (a corner shared by several cells of
// the unit gets one global add per cell: coarse levels have few cells per unit).
__device__ __forceinline__ uint32_t sc_corner_entry(const ScLevel& L, uint32_t px, uint32_t py, uint32_t pz, int c) {
    const uint32_t x = px + (c & 1), y = py + ((c >> 1) & 1), z = pz + ((c >> 2) & 1);
    if (L.dense) {
        const uint32_t e = x + L.res * y + L.res * L.res * z;
        return e < L.params ? e : e % L.params;
    }
    return (x ^ (y * 2654435761u) ^ (z * 805459861u)) & (L.params - 1);
}

// A lane's run of consecutive samples in one cell of a coarse level: the 8 corners' weighted sums
// in registers, carried over the lane's chunks of a unit; a finished run goes to the wave's queue
// (sc_push_run), whose full-wave passes add the runs to the cell table (sc_drain_cells).
struct ScRun {
    uint32_t px, py, pz;
    bool any, init;
    float v[16];
};

// The wave's queued runs [0, qn) into the cell table, one run per lane: one set read and claim per
// run, the 16 sums as fixed-point ds_add_u64 in four float4 groups; a run whose set is full goes to
// global f32 atomics.
__device__ __forceinline__ void sc_drain_cells(ScShared& sh, int lane, const uint32_t* qk, const float4* qv, int qn,
                                               const ScLevel& L, float* __restrict__ grad) {
    asm volatile("" ::: "memory");  // (the wave's queue writes come first: a wave's LDS operations execute in order)
    SC_TNOW(td0);
    const bool act = lane < qn;
    const uint32_t key = act ? qk[lane] : 0u;
    const int p0 = SC_WAYS * (int)sc_set(key, sh.sets);
    int sl = -1;
    bool isnew = false;
    uint4 kk = make_uint4(0u, 0u, 0u, 0u);
    if (act) {
        kk = *(const uint4*)&sh.keys[p0];
        sl = kk.x == key ? p0 : kk.y == key ? p0 + 1 : kk.z == key ? p0 + 2 : kk.w == key ? p0 + 3 : -1;
    }
    if (__ballot(act && sl < 0)) {  // uniform: some lane claims
        if (act && sl < 0) {
#pragma unroll
            for (int attempt = 0; attempt < 2 && sl < 0; attempt++) {
                if (attempt) {  // lost a claim: look again
                    asm volatile("" ::: "memory");
                    kk = *(const uint4*)&sh.keys[p0];
                    sl = kk.x == key ? p0 : kk.y == key ? p0 + 1 : kk.z == key ? p0 + 2 : kk.w == key ? p0 + 3 : -1;
                    if (sl >= 0) break;
                }
                const int cl = kk.x == SC_EMPTY ? p0 : kk.y == SC_EMPTY ? p0 + 1 : kk.z == SC_EMPTY ? p0 + 2
                             : kk.w == SC_EMPTY ? p0 + 3 : -1;
                if (cl < 0) break;  // set full
                const uint32_t got = atomicCAS(&sh.keys[cl], SC_EMPTY, key);
                if (got == SC_EMPTY) { sl = cl; isnew = true; }
                else if (got == key) sl = cl;
            }
        }
    }
    const bool fb = act && sl < 0;
    const bool anyfb = __ballot(fb) != 0;  // uniform: a set full of other cells
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const float4 v = act ? qv[4 * lane + g] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int h = 0; h < 4; h++) {
            const int j = 4 * g + h;  // corner j / 2, component j % 2
            if (act && sl >= 0)
                atomicAdd((unsigned long long*)&sh.valx[j * sh.slots + sl], (unsigned long long)sc_fix(vv[h], L.k));
        }
        if (anyfb && fb) {
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const int j = 4 * g + h;
                const uint32_t e = L.off + sc_corner_entry(L, key & 2047u, (key >> 11) & 2047u, key >> 22, j >> 1);
                if (vv[h] != 0.f) atomicAdd(grad + 2 * (size_t)e + (j & 1), vv[h]);
            }
        }
    }
    // append the claimed slots to `used`: one LDS atomic per wave
    const uint64_t nm = __ballot(isnew);
    if (nm) {
        int base = 0;
        if (lane == 0) base = atomicAdd(sh.fill, (int)__popcll(nm));
        base = __builtin_amdgcn_readfirstlane(base);
        if (isnew)
            sh.used[base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(nm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nm, 0))] =
                (uint16_t)sl;
    }
    asm volatile("" ::: "memory");  // (the queue is rewritten after these reads)
    SC_TWAIT();
    SC_TNOW(td1);
    SC_TADDC(2, td0, td1);
}

// Queue the finished runs of the lanes with `fin` (whole wave calls; qn wave-uniform): a full queue
// is drained first.  Cells outside the key range go straight to global memory.
__device__ __forceinline__ void sc_push_run(ScShared& sh, int lane, bool fin, const ScRun& st, uint32_t* qk, float4* qv,
                                            int& qn, const ScLevel& L, float* __restrict__ grad) {
    // (pz < 1023: the key of cell (2047, 2047, 1023) would be SC_EMPTY — a lookup would then "find" it
    // in any empty way, add into a slot that is never claimed nor flushed, and leave the sums behind
    // for the slot's next owner)
    const bool inkey = st.px < 2048u && st.py < 2048u && st.pz < 1023u;
    const uint64_t bm = __ballot(fin && inkey);
    if (bm) {
        const int n = (int)__popcll(bm);
        if (qn + n > SC_QUEUE) {
            sc_drain_cells(sh, lane, qk, qv, qn, L, grad);
            qn = 0;
        }
        if (fin && inkey) {
            const int p = qn + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0));
            qk[p] = st.px | (st.py << 11) | (st.pz << 22);
#pragma unroll
            for (int g = 0; g < 4; g++)
                qv[4 * p + g] = make_float4(st.v[4 * g], st.v[4 * g + 1], st.v[4 * g + 2], st.v[4 * g + 3]);
        }
        qn += n;
    }
    if (__ballot(fin && !inkey)) {  // uniform: (not on the configs' levels) straight to global memory
        if (fin && !inkey) {
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const uint32_t e = L.off + sc_corner_entry(L, st.px, st.py, st.pz, c);
                if (st.v[2 * c] != 0.f) atomicAdd(grad + 2 * (size_t)e, st.v[2 * c]);
                if (st.v[2 * c + 1] != 0.f) atomicAdd(grad + 2 * (size_t)e + 1, st.v[2 * c + 1]);
            }
        }
    }
}
template <int C>
__device__ __forceinline__ void sc_cells_run(ScShared& sh, int lane, const ScChunk<C>& ch, const ScLevel& L,
                                             float* __restrict__ grad, ScRun& st, bool last, uint32_t* qk, float4* qv,
                                             int& qn) {
#pragma unroll
    for (int i = 0; i < C; i++) {
        const LevelPos q = level_pos(L.scale, ch.x[i], ch.y[i], ch.z[i]);
        const bool change = st.init && (q.px != st.px || q.py != st.py || q.pz != st.pz);
        sc_push_run(sh, lane, change && st.any, st, qk, qv, qn, L, grad);
        if (change || !st.init) {
#pragma unroll
            for (int j = 0; j < 16; j++) st.v[j] = 0.f;
            st.any = false;
            st.px = q.px; st.py = q.py; st.pz = q.pz;
            st.init = true;
        }
        st.any = st.any || ch.g[i].x != 0.f || ch.g[i].y != 0.f;
        sc_corner_sums(q, ch.g[i], st.v);
    }
    if (last) {  // the unit's last runs, then the rest of the queue
        sc_push_run(sh, lane, st.any, st, qk, qv, qn, L, grad);
        if (qn) sc_drain_cells(sh, lane, qk, qv, qn, L, grad);
        qn = 0;
    }
}

// Flush of a cell unit: 16 lanes per claimed cell (one corner component each), form the corner's
// entry, f32 global adds; lane 0 of the cell resets the key, each lane its value.
__device__ __forceinline__ void sc_flush_cells(ScShared& sh, const ScLevel& L, float* __restrict__ grad) {
    const int nf = *sh.fill;
    constexpr int V = SC_CELL_VALS;
    for (int i = threadIdx.x; i < V * nf; i += SC_THREADS) {
        const int slot = sh.used[i / V], j = i % V;
        const uint32_t key = sh.keys[slot];
        long long* pv = &sh.valx[j * sh.slots + slot];
        const long long q = *pv;
        *pv = 0;
        if (q != 0) {
            const uint32_t e = L.off + sc_corner_entry(L, key & 2047u, (key >> 11) & 2047u, key >> 22, j >> 1);
            atomicAdd(grad + 2 * (size_t)e + (j & 1), (float)ldexp((double)q, -L.k));
        }
        if (j == 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the cell's other lanes have read the key: same wave)
            sh.keys[slot] = SC_EMPTY;
        }
    }
}

__device__ __forceinline__ ScLevel sc_level(const LevelTable& Lt, int l, float m, int kbase) {
    ScLevel L;
    L.scale = Lt.scale[l];
    L.res = Lt.res[l];
    L.params = Lt.params[l];
    L.off = Lt.offset[l];
    L.dense = (uint64_t)L.res * L.res * L.res <= L.params;  // tcnn: stride stays <= params
    L.direct = !isfinite(m);  // (uniform) non-finite gradient: every corner straight to global memory
    int e2 = 0;
    (void)frexpf(L.direct ? 1.f : m, &e2);  // m < 2^e2
    // |sum| <= (unit samples) * m * 2^k + rounding (a sample's 8 corner weights sum to 1): < 2^62,
    // and every addend (a run's corner sum) < 2^51, sc_fix's range (the callers' kbase)
    L.k = kbase - e2;
    return L;
}

// The next unit of the workgroup (field_scatter_kernel's queue): thread 0 draws it when its samples
// are done (few live registers there; the atomic's return is hidden behind the unit's barrier wait
// and flush) and publishes it in LDS before the unit's closing barrier.
struct ScDraw {
    unsigned* queue;
    int* slot;
};

// One fine-level unit of 1024 x C samples: the samples in grabs, then the flush of the claimed slots.
// (C is a run-time value: one inlined copy of the grab loop serves every fine level.)
__device__ __forceinline__ void sc_unit(ScShared& sh, int wid, int lane, int l, int C, int64_t s0, int64_t s1,
                                        const float* __restrict__ xyzs, const uint32_t* __restrict__ dEl,
                                        const ScDE& de, const ScNorm& nrm, const LevelTable& Lt, float m, float* __restrict__ grad,
                                        const int32_t* __restrict__ order, bool perm, const ScDraw& draw) {
    SC_TNOW(t0);
    // (a fine unit holds at most 4096 samples: 2^46 leaves the sums four bits of headroom below 2^62)
    const ScLevel L = sc_level(Lt, l, m, 46);
    SC_TNOW(t1);
    // The unit's 1024 x C samples in grabs of 64 lanes x 2: grab k gives lane t the samples
    // s0 + (t * NG + k) * 2 — the 64 lanes of one wave-instruction hold samples 2 * NG positions
    // apart, so they rarely address the same LDS slot at once (same-address LDS atomics
    // serialise).  Wave w takes grab w first, then draws grabs from the unit's LDS counter after
    // each grab's adds, so a wave slowed by claims / set-full fallbacks takes fewer grabs and the
    // waves reach the unit's barrier together (191 vs 195 us static; drawing one grab ahead so
    // that its loads overlap spills 9 VGPRs: 194).  Round 5: level 15's 2048-sample units go through
    // the same loop (16 grabs for 16 waves: the assignment of the former static 2-sample chunks; one
    // code path, 186-188 vs 189-190 us in the probe); 1-sample grabs (finer balance, shorter runs) on
    // levels 13-15 were no better.
    const int NG = SC_THREADS * C / 128;
    int k = wid;
    ScChunk<2> cg;
    // (positions: the class array holds grab k's 64 chunks of 2 side by side, sc_perm)
#define SC_GRAB_S(k) (s0 + ((int64_t)lane * NG + (k)) * 2)
#define SC_GRAB_P(k) (perm ? s0 + ((int64_t)(k) * 64 + lane) * 2 : SC_GRAB_S(k))
    sc_load_chunk<2>(cg, SC_GRAB_S(k), SC_GRAB_P(k), s1, xyzs, dEl, de, nrm, order);
    while (k < NG) {  // (wave-uniform)
        sc_direct<2>(sh, lane, cg, L, grad);
        int kn = 0;
        if (lane == 0) kn = atomicAdd(sh.grab, 1);
        kn = __builtin_amdgcn_readfirstlane(kn) + SC_WAVES;
        if (kn < NG) sc_load_chunk<2>(cg, SC_GRAB_S(kn), SC_GRAB_P(kn), s1, xyzs, dEl, de, nrm, order);
        k = kn;
    }
    SC_TNOW(t2);
#ifdef NCN_DIAG_SC_TIMES
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (diagnostic: the wave's own LDS ops drain)
#endif
    SC_TNOW(t2b);
    unsigned next = 0;
    if (threadIdx.x == 0) next = atomicAdd(draw.queue, 1u);  // (its return waits behind the barrier and the flush)
    lds_barrier();
    SC_TNOW(t3);
    // flush: the claimed slots, two lanes per slot (x and y of one entry are adjacent floats, one
    // 8-B piece of one 64-B granule per lane pair); each lane resets the half it read (the even
    // lane the key and x, the odd one y), so one barrier closes the unit
    const int nf = *sh.fill;
    for (int i = threadIdx.x; i < 2 * nf; i += SC_THREADS) {
        const int slot = sh.used[i >> 1];
        const uint32_t key = sh.keys[slot];
        long long* pv = (i & 1) ? &sh.valy[slot] : &sh.valx[slot];
        const float gv = (float)ldexp((double)*pv, -L.k);
        *pv = 0;
        if (gv != 0.f) atomicAdd(grad + 2 * (size_t)(L.off + key) + (i & 1), gv);
        if (!(i & 1)) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the odd lane has read the key: same wave)
            sh.keys[slot] = SC_EMPTY;
        }
    }
    if (threadIdx.x == 0) *draw.slot = (int)next;
    lds_barrier();
    SC_TNOW(t4);
    SC_TADD(0, t0, t1);
    SC_TADD(1, t1, t2);
    SC_TADD(2, t2, t2b);
    SC_TADD(3, t2b, t3);
    SC_TADD(4, t3, t4);
}

// Cell units: 1024 x C x `rounds` consecutive samples, then one flush.  Lane t of wave w takes the
// unit's (t * SC_WAVES + w)-th slice of C x rounds consecutive samples (neighbouring slices in
// different waves), a chunk of C per round, and carries its current run over the rounds, so a run
// ends only where the samples leave the cell.  Rounds per level: coarse levels have few cells, so
// longer units mean fewer flushes and barriers.  (Round 5: carried runs with the next chunk loaded
// at the top of the round, no prefetch: levels 0-9 95 -> 75 us, all levels 201 -> 192 us; with the
// prefetch the carried state spilled 18 VGPRs: 199 us.)
template <int C>
__device__ __forceinline__ void sc_cell_unit(ScShared& sh, int wid, int lane, int l, int64_t s0, int64_t s1, int rounds,
                                             const float* __restrict__ xyzs, const uint32_t* __restrict__ dEl,
                                             const ScDE& de, const ScNorm& nrm, const LevelTable& Lt, float m, float* __restrict__ grad,
                                             const int32_t* __restrict__ order, bool perm, const ScDraw& draw) {
    const int lg_unit = (31 - __builtin_clz(SC_THREADS * C)) + (31 - __builtin_clz((unsigned)rounds));
    // scale 2^k, k = 60 - lg_unit - e: the unit's sum of every corner stays below 2^61, and one run
    // (at most rounds x C <= 2^(lg_unit - 10) samples) below 2^(50) — sc_fix needs |addend| < 2^51
    const ScLevel L = sc_level(Lt, l, m, 60 - lg_unit);
    const int64_t lane_off = ((int64_t)lane * SC_WAVES + wid) * rounds * C;
    ScRun st;
    st.init = st.any = false;
    st.px = st.py = st.pz = 0;
    uint32_t* qk = sh.qkey + wid * SC_QUEUE;  // (this wave's run queue)
    float4* qv = sh.qval + wid * SC_QUEUE * 4;
    int qn = 0;
    for (int r = 0; r < rounds; r++) {
        ScChunk<C> ch;
        // (positions: the class array holds a round's 64 chunks of a wave side by side, sc_perm)
        const int64_t sb = s0 + lane_off + (int64_t)r * C;
        SC_TNOW(tc0);
        sc_load_chunk<C>(ch, sb, perm ? s0 + (((int64_t)r * SC_WAVES + wid) * 64 + lane) * C : sb, s1, xyzs, dEl, de, nrm,
                         order);
        SC_TWAIT();
        SC_TNOW(tc1);
        SC_TADDC(0, tc0, tc1);
        if (L.direct)
            sc_direct<C>(sh, lane, ch, L, grad);  // (sc_add's direct form: f32 global adds, NaN/Inf propagate)
        else
            sc_cells_run<C>(sh, lane, ch, L, grad, st, r + 1 == rounds, qk, qv, qn);
        SC_TWAIT();
        SC_TNOW(tc2);
        SC_TADDC(1, tc1, tc2);  // (run work including the drains, which add to slot 2 as well)
    }
    SC_TNOW(tc3);
    unsigned next = 0;
    if (threadIdx.x == 0) next = atomicAdd(draw.queue, 1u);  // (its return waits behind the barrier and the flush)
    lds_barrier();
    SC_TNOW(tc4);
    sc_flush_cells(sh, L, grad);
    if (threadIdx.x == 0) *draw.slot = (int)next;
    lds_barrier();
    SC_TNOW(tc5);
    SC_TADDC(3, tc3, tc4);
    SC_TADDC(4, tc4, tc5);
}

// The sample positions in the permuted order of each class the scatter needs (class_mask), into
// the dE workspace behind the encoding gradient: a thread takes 4 consecutive samples (one 48-B
// piece in, one 48-B coarse chunk / two 24-B fine pairs out per class).
__global__ __launch_bounds__(256) void sc_perm_positions_kernel(const float* __restrict__ xyzs, int64_t n_stride,
                                                                const int32_t* __restrict__ n_dev, int class_mask,
                                                                float* __restrict__ xyz_perm, float* __restrict__ flag,
                                                                float flag_value) {
    const int64_t n = n_dev ? min<int64_t>(n_stride, *n_dev) : n_stride;
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = flag_value;
    // (xyz_perm: the workspace's class 0 array, flag: its POS_MASK word; whole units: n's rounding to 4 changes nothing)
    const int64_t ps = sc_perm_stride(n_stride);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; 4 * j < n; j += (int64_t)gridDim.x * 256) {
        const int64_t sb = 4 * j;
        float v[12];
        if (sb + 4 <= n) {
            const float4* px = (const float4*)(xyzs + 3 * sb);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const float4 f = px[q];
                v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 12; i++) v[i] = sb + i / 3 < n ? xyzs[3 * sb + i] : 0.f;
        }
#pragma unroll
        for (int cls = 0; cls < SC_N_CLASSES; cls++) {
            if (!((class_mask >> cls) & 1)) continue;
            float* out = xyz_perm + DeWs::class_offset(cls, ps);
            if (cls < 2) {  // the 4 samples are one chunk
                float4* po = (float4*)(out + 3 * sc_perm(sb, cls));
                po[0] = make_float4(v[0], v[1], v[2], v[3]);
                po[1] = make_float4(v[4], v[5], v[6], v[7]);
                po[2] = make_float4(v[8], v[9], v[10], v[11]);
            } else {  // two pairs
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    float2* po = (float2*)(out + 3 * sc_perm(sb + 2 * h, cls));
                    po[0] = make_float2(v[6 * h], v[6 * h + 1]);
                    po[1] = make_float2(v[6 * h + 2], v[6 * h + 3]);
                    po[2] = make_float2(v[6 * h + 4], v[6 * h + 5]);
                }
            }
        }
    }
}

// One unit u of the scatter (see field_scatter_kernel): its level, span and layout.
__device__ __forceinline__ bool sc_one_unit(int64_t u, int64_t n, const int* unit_start, const int* unit_level, int& layout,
                                            int& par, const ScDraw& draw, ScShared& sh,
                                            char* arena, int* fill, const float* lmax_s, int wid, int lane,
                                            const float* __restrict__ xyzs, const float* __restrict__ pos, int perm_mask,
                                            const uint32_t* __restrict__ dE, const DeWs& ws, const ScDE& de, const ScNorm& nrm, const LevelTable& Lt,
                                            float* __restrict__ grad, const int32_t* __restrict__ order) {
    int i = 0;  // (uniform) unit u is unit v of level l
    while (i < 15 && u >= unit_start[i + 1]) i++;
    const int l = unit_level[i];
    const int64_t v = u - unit_start[i], span = sc_unit_span(l);
    const int64_t s0 = v * span, s1 = min(n, s0 + span);
    const int mode = l < SC_CELL_HI ? SC_MODE_CELL : SC_MODE_DIR;
    if (mode != layout) {  // (re)initialise the table of the new layout
        lds_barrier();
        sh = sc_layout(arena, fill, mode);
        const int nv = mode == SC_MODE_CELL ? SC_CELL_VALS * sh.slots : 2 * sh.slots;
        for (int i = threadIdx.x; i < sh.slots; i += SC_THREADS) sh.keys[i] = SC_EMPTY;
        for (int i = threadIdx.x; i < nv; i += SC_THREADS) sh.valx[i] = 0;
        if (threadIdx.x == 0) fill[0] = fill[1] = fill[2] = fill[3] = 0;
        lds_barrier();
        layout = mode;
        par = 0;
    }
    float m = lmax_s[l];
#ifdef NCN_DIAG_SC_LEVELS_MASK
    if (!((NCN_DIAG_SC_LEVELS_MASK >> l) & 1)) m = 0.f;  // diagnostic: skip this level
#endif
    if (m == 0.f) return false;  // uniform: nothing to add on this level (no barrier, parity kept; no draw)
    // the unit claims into fill[par]; fill[par ^ 1] (read by every lane before the previous
    // unit's closing barrier) is reset here for the next unit
    sh.fill = fill + par;
    sh.grab = fill + 2 + par;  // (the grab counters behind the claim counts, alternating alike)
    if (threadIdx.x == 0) { fill[par ^ 1] = 0; fill[2 + (par ^ 1)] = 0; }
    par ^= 1;
    const uint32_t* dEl = dE + (int64_t)l * ws.e_stride;
    // (positions: the level's class array, or the sample-ordered ones)
    const bool perm = (perm_mask >> sc_class(l)) & 1;
    if (perm) xyzs = pos + ws.class_offset(sc_class(l));
    if (mode == SC_MODE_CELL)
        sc_cell_unit<SC_C_CELL>(sh, wid, lane, l, s0, s1, sc_cell_rounds(l), xyzs, dEl, de, nrm, Lt, m, grad, order, perm,
                                draw);
    else
        sc_unit(sh, wid, lane, l, sc_fine_c(l), s0, s1, xyzs, dEl, de, nrm, Lt, m, grad, order, perm, draw);
    return true;
}

// (ncn_field_scatter_wgrad) the MLP weight-gradient slab rows summed into gw, in SC_WGRAD_SLICES
// contiguous slices of the weights, one per queue entry behind the table units (so the workgroups that
// finish their table units first take them; round 6: the reduction at the start of every workgroup
// delayed all units by its duration): the threads of a slice take (weight, 16-row chunk) pairs with
// the weight varying fastest (coalesced rows); one f32 atomic per pair, as reduce_wgrad_kernel.
constexpr int SC_WGRAD_SLICES = 256;
__device__ __forceinline__ void sc_wgrad_slice(int slice, const float* __restrict__ wslab, int nb_sigma, int nb_rgb,
                                               float* __restrict__ gw) {
    const int per = (NCN_FIELD_NW + SC_WGRAD_SLICES - 1) / SC_WGRAD_SLICES;
    const int w0 = slice * per, nw = min(NCN_FIELD_NW, w0 + per) - w0;
    const int chunks = (max(nb_sigma, nb_rgb) + WRED_CHUNK - 1) / WRED_CHUNK;
    for (int idx = threadIdx.x; idx < nw * chunks; idx += SC_THREADS) {
        const int w = w0 + idx % nw, c = idx / nw;
        const int nb = w < W3_OFF ? nb_sigma : nb_rgb;
        const int b1 = min(nb, (c + 1) * WRED_CHUNK);
        float acc = 0.f;
        for (int b = c * WRED_CHUNK; b < b1; b++) acc += wslab[(int64_t)b * NCN_FIELD_NW + w];
        if (c * WRED_CHUNK < nb) atomicAdd(gw + w, acc);
    }
}

__global__ __launch_bounds__(SC_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void field_scatter_kernel(const float* __restrict__ xyzs, int64_t n_stride,
                                                                   const int32_t* __restrict__ n_dev, LevelTable Lt,
                                                                   float xyz_min, float xyz_extent,
                                                                   const float* __restrict__ dE_ws,
                                                                   float* __restrict__ grad,
                                                                   const float* __restrict__ level_max, int lm_rows,
                                                                   int level_lo, int level_hi,
                                                                   const int32_t* __restrict__ order,
                                                                   const float* __restrict__ wslab = nullptr,
                                                                   int nb_sigma = 0, int nb_rgb = 0,
                                                                   float* __restrict__ gw = nullptr,
                                                                   unsigned* __restrict__ queue = nullptr) {
    __shared__ __attribute__((aligned(16))) char arena[SC_ARENA];
    __shared__ int fill[4];  // claimed-slot counts [0, 2) and grab counters [2, 4), alternating per unit (reset one unit ahead)
    // per-level max |dE| over the MLP pass's workgroup rows (the fixed-point scale of each level);
    // visible to every thread at the first layout barrier
    __shared__ float lmax_s[16];
    // the launch's levels in order: unit_start[i] = the first unit of the i-th of them (padded with
    // the unit count to 16), unit_level[i] its level
    __shared__ int unit_start[17], unit_level[16];
    const int64_t n = n_dev ? min<int64_t>(n_stride, *n_dev) : n_stride;
    if (threadIdx.x < 16) lmax_s[threadIdx.x] = 0.f;
    if (threadIdx.x == 0) {
        int acc = 0, k = 0;
        for (int l = level_lo; l < level_hi; l++) {
            unit_start[k] = acc;
            unit_level[k++] = l;
            acc += (int)((n + sc_unit_span(l) - 1) / sc_unit_span(l));
        }
        for (; k < 17; k++) unit_start[k] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < lm_rows * 16; i += SC_THREADS)  // one load per thread, LDS max
        atomicMax((unsigned*)&lmax_s[i & 15], __float_as_uint(level_max[i]));  // (non-negative floats)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#ifdef NCN_DIAG_SC_SPAN
    if (threadIdx.x == 0 && blockIdx.x < 256) {
        ncn_sc_span[blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
        ncn_sc_span[blockIdx.x][2] = __builtin_readcyclecounter();
    }
#endif
    const DeWs ws(n_stride);  // the MLP pass's dE workspace (field_de_ws.h)
    ScNorm nrm;
    nrm.mn = xyz_min;
    nrm.ext = xyz_extent;
    nrm.inv = 1.0f / xyz_extent;
    nrm.pow2 = (__float_as_uint(xyz_extent) & 0x807FFFFFu) == 0u && xyz_extent > 0.f;
    ScDE de;
    de.inv = dE_ws[DeWs::INV_S];
    de.bf16 = dE_ws[DeWs::OPERAND] != 0.f;
    // positions: a unit class's permuted copy when the MLP pass (or ncn_field_scatter_positions)
    // wrote it (header mask), else the sample-ordered xyzs (strided loads)
    const int perm_mask = order ? 0 : (int)dE_ws[DeWs::POS_MASK];
    const uint32_t* dE = (const uint32_t*)(dE_ws + ws.row(0));  // [16][e_stride] pairs
    const float* pos = dE_ws + ws.positions();
    // units of the levels [level_lo, level_hi), sc_unit_span(l) samples each: cell levels
    // [0, SC_CELL_HI) in spans of 1024 * C_CELL * rounds(l), fine levels 1024 * sc_fine_c(l)
    const int64_t n_units = unit_start[16], n_all = n_units + (wslab ? SC_WGRAD_SLICES : 0);
    // Units level-major (the cell levels' long units first): workgroup b takes unit b first, then draws
    // the next from the launch's queue — at the end of each unit's samples (ScDraw), so the draw's
    // return is hidden behind the unit's barrier wait and flush.  A workgroup's units go cell -> fine:
    // at most one layout switch.  (Round 6: the static stride b, b + gridDim.x, ... left the
    // workgroups' ends spread over 94-169 us for a mean of 142 us of work — about five units of 20-55
    // us each, profiles/round6/scatter_probe_span.log; with the queue 130-159 us and the scatter 175.8
    // -> 164-165 us, scatter_probe_queue_dynamic.log.  Fine levels drawn in cost order instead of
    // level-major, or coarse units of half the samples, measured no better: scatter_probe_order.log.)
    int layout = -1, par = 0;
    ScShared sh;
    __shared__ int next_unit[2];  // (alternating: a slot is rewritten only after a barrier every reader passed)
#ifdef NCN_DIAG_SC_SPAN
    int diag_k = 0;
#endif
    int64_t u = blockIdx.x;
    for (int qpar = 0; u < n_all; qpar ^= 1) {  // (uniform)
        ScDraw draw;
        draw.queue = queue;
        draw.slot = next_unit + qpar;
        bool drew = false;
        if (u < n_units)
            drew = sc_one_unit(u, n, unit_start, unit_level, layout, par, draw, sh, arena, fill, lmax_s, wid, lane, xyzs, pos,
                               perm_mask, dE, ws, de, nrm, Lt, grad, order);
        else
            sc_wgrad_slice((int)(u - n_units), wslab, nb_sigma, nb_rgb, gw);
#ifdef NCN_DIAG_SC_SPAN
        if (threadIdx.x == 0 && blockIdx.x < 256 && diag_k < 8) {
            ncn_sc_span[blockIdx.x][4 + 2 * diag_k] = (unsigned long long)u;
            ncn_sc_span[blockIdx.x][5 + 2 * diag_k] = __builtin_amdgcn_s_memrealtime();
        }
        diag_k++;
#endif
        if (!drew) {  // (uniform) a skipped unit: draw here
            if (threadIdx.x == 0) next_unit[qpar] = (int)atomicAdd(queue, 1u);
            __syncthreads();
        }
        u = (int64_t)next_unit[qpar] + gridDim.x;
    }
    // the last workgroup out leaves the queue zero for the next launch on this workspace (every
    // workgroup has made its last draw before it departs)
    if (threadIdx.x == 0 && atomicAdd(queue + 1, 1u) == gridDim.x - 1) {
        __hip_atomic_store(queue, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(queue + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#ifdef NCN_DIAG_SC_SPAN
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < 256) {
        ncn_sc_span[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
        ncn_sc_span[blockIdx.x][3] = __builtin_readcyclecounter();
    }
#endif
}
}  // namespace ncn
