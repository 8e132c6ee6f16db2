// The dE workspace between the passes of the field backward, and the scatter geometry it is laid out by:
// ncn_field_bwd_dE_floats(n) floats, 16-byte aligned, n = the sample capacity (DeWs below):
//   header     4 floats: [INV_S] 1 / S of the fp16 chain's loss scale, [OPERAND] 0 fp16 / 1 bf16,
//              [POS_MASK] the mask of unit classes whose permuted positions the workspace holds, one spare
//   rows       [16][e_stride] level-major pairs of the operand type, one 4-byte word per sample
//              (e_stride = n rounded up to 4: 16-byte aligned rows)
//   positions  SC_N_CLASSES arrays of 3 * pos_stride floats: the samples' xyz in the load order of
//              the class's units (sc_perm; pos_stride = e_stride rounded up to whole longest units)
//   queue      SC_QUEUE_WORDS words: per level_lo of a scatter launch a grab and a departure counter
// Who writes what (field_bwd_kernel's parts: rgb, sigma, or both in one pass):
//   INV_S, OPERAND, rows, queue = 0   the sigma pass and the one-pass form
//   POS_MASK, positions               the rgb pass and the one-pass form: classes [0, DE_POS_MLP_CLASSES)
//                                     (mask 0 and no positions under a processing order);
//                                     ncn_field_scatter_positions: all SC_N_CLASSES
// Readers: field_scatter_kernel (all four parts; leaves the queue zero), field_bwd_dx_kernel (header, rows).
// Caveat: POS_MASK is rewritten by those three writers only.  A sigma pass on its own, or a scatter
// after the sample positions changed without one of them, finds the last writer's mask and positions.
// The workspace is sized for all SC_N_CLASSES position arrays although the MLP pass writes two.
#pragma once
#include "common.h"
namespace ncn {
// ---- scatter geometry (field_scatter.h): what the layout and the MLP pass's position writes need ----
constexpr int SC_THREADS = 1024;  // one workgroup per CU (the LDS table takes the CU's LDS)
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_CELL_HI = 10;    // levels [0, SC_CELL_HI) are cell-keyed, the rest entry-keyed
// Samples per lane of a fine-level unit (unit = 1024 x C samples): 4 (4096-sample units, in grabs of
// 64 x 2) up to level 14; level 15 takes 2 (its ~1 distinct entry per sample would overfill the
// 4-way sets of a 4096-sample unit; units of 2048 from level 13: 198, 14: 202, 15: 190, none: 202 us).
// (Measured round 5: 8192-sample units on levels 10-11 / 10-12: 288 / 281 us against 202; two
// 512-thread workgroups per CU with half the table each: slower.)
__host__ __device__ constexpr int sc_fine_c(int l) { return l < 15 ? 4 : 2; }
// Tuning switches: samples per lane per round on the cell levels, a cell unit's rounds on levels 0-5 / 6-9.
#ifndef NCN_SC_C_CELL
#define NCN_SC_C_CELL 4
#endif
#ifndef NCN_SC_R_LO
#define NCN_SC_R_LO 8
#endif
#ifndef NCN_SC_R_MID
#define NCN_SC_R_MID 4
#endif
constexpr int SC_C_CELL = NCN_SC_C_CELL;
__host__ __device__ constexpr int sc_cell_rounds(int l) { return l < 6 ? NCN_SC_R_LO : l < 10 ? NCN_SC_R_MID : 1; }
// samples of one unit of level l
__host__ __device__ constexpr int64_t sc_unit_span(int l) {
    return (int64_t)SC_THREADS * (l < SC_CELL_HI ? SC_C_CELL * sc_cell_rounds(l) : sc_fine_c(l));
}

// Unit classes by the sample layout their loads use: coarse levels 0-5 (rounds NCN_SC_R_LO) and 6-9
// (NCN_SC_R_MID), fine levels 10-14 (C = 4) and 15 (C = 2).
constexpr int SC_N_CLASSES = 4;
__host__ __device__ constexpr int sc_class(int l) { return l < 6 ? 0 : l < SC_CELL_HI ? 1 : l < 15 ? 2 : 3; }
constexpr int64_t SC_MAX_SPAN = (int64_t)SC_THREADS * SC_C_CELL * NCN_SC_R_LO;
static_assert(sc_cell_rounds(0) == NCN_SC_R_LO && NCN_SC_R_LO >= NCN_SC_R_MID && sc_fine_c(10) <= SC_C_CELL, "spans");
// the permuted positions' row length (every class array holds whole units)
__host__ __device__ constexpr int64_t sc_perm_stride(int64_t n_stride) {
    return (n_stride + SC_MAX_SPAN - 1) / SC_MAX_SPAN * SC_MAX_SPAN;
}
// Where sample s sits in its class's permuted position array: the samples a wave loads in one
// instruction lie side by side, so a coarse round or a fine grab reads one contiguous stretch
// (coalesced) while each lane keeps its own consecutive samples (the runs).  Coarse: lane t of wave
// w owns the unit's slice t * 16 + w of 4R samples and reads chunk r in round r; fine: lane t reads
// the pair t * NG + k in grab k.  A chunk (4 coarse / 2 fine samples) stays contiguous.
__device__ __forceinline__ int64_t sc_perm(int64_t s, int cls) {
    if (cls < 2) {
        const int R = sc_cell_rounds(cls == 0 ? 0 : 6), CR = SC_C_CELL * R;
        const int64_t U = (int64_t)SC_THREADS * CR, o = s % U;
        const int64_t slice = o / CR, within = o % CR;
        const int64_t t = slice / SC_WAVES, w = slice % SC_WAVES, r = within / SC_C_CELL, i = within % SC_C_CELL;
        return (s - o) + ((r * SC_WAVES + w) * 64 + t) * SC_C_CELL + i;
    }
    const int C = sc_fine_c(cls == 2 ? 10 : 15), NG = SC_THREADS * C / 128;
    const int64_t U = (int64_t)SC_THREADS * C, o = s % U;
    const int64_t pair = o >> 1, t = pair / NG, k = pair % NG;
    return (s - o) + (k * 64 + t) * 2 + (o & 1);
}

// The table scatter's unit queue: zeroed by the MLP pass that writes the header, and left zero by
// every scatter launch (its last workgroup out resets the counters).
constexpr int SC_QUEUE_WORDS = 32;
// The MLP pass writes the coarse classes' positions only: the coarse units' strided loads cost
// 16-20 us per unit, the fine units' grabs measured no faster from permuted positions (round 6,
// profiles/round6/scatter_probe_perm.log), and the writes run beside the clustering.
constexpr int DE_POS_MLP_CLASSES = 2;
// The pass that writes them: the rgb pass, beside the clustering (round 6 A/B against the sigma pass
// after the join: 14.28 / 14.29 M rays/s alike).
constexpr int DE_POS_PART = 1;  // BWD_RGB

// The layout for a capacity of n samples: offsets in floats from the workspace's start.
struct DeWs {
    enum { INV_S = 0, OPERAND = 1, POS_MASK = 2, HEADER_FLOATS = 4 };
    int64_t e_stride;
    __host__ __device__ explicit DeWs(int64_t n) : e_stride((n + 3) & ~(int64_t)3) {}
    // (a function, not a member set in the constructor: the kernels compute it on their position paths,
    // and one that wants it once keeps it in a local for the static class_offset)
    __host__ __device__ int64_t pos_stride() const { return sc_perm_stride(e_stride); }
    __host__ __device__ int64_t row(int l) const { return HEADER_FLOATS + l * e_stride; }
    __host__ __device__ static int64_t class_offset(int cls, int64_t pos_stride) { return cls * 3 * pos_stride; }
    __host__ __device__ int64_t class_offset(int cls) const { return cls * 3 * pos_stride(); }  // from class 0's array
    __host__ __device__ int64_t positions() const { return row(16); }  // class 0's array (no stride needed)
    __host__ __device__ int64_t positions(int cls) const { return positions() + class_offset(cls); }
    __host__ __device__ int64_t queue() const { return positions(SC_N_CLASSES); }
    __host__ __device__ int64_t floats() const { return queue() + SC_QUEUE_WORDS; }
};
}  // namespace ncn
