// Diagnostic builds of the field backward (tools/build_field_variants.sh): the probes' macro tables, device
// arrays and exports.  The probe points stay in the kernels; in a product build every macro here is empty.
#pragma once
#include "common.h"
namespace ncn {
// NCN_DIAG_SIGMA_TIMES (tools/sigma_pass_probe.py) records, per workgroup of the
// sigma pass, wave 0's cycles summed over its steps — waiting on the prefetched loads, phase 1, the
// first barrier, phase 2, the second barrier — the step count, and the realtime clock (100 MHz) at
// the kernel's entry, before the first step, after the last and at the exit.
#ifdef NCN_DIAG_SIGMA_TIMES
__device__ unsigned long long ncn_sigma_times[512][10];
#define SG_TNOW(v) const unsigned long long v = __builtin_readcyclecounter()
#define SG_TADD(i, a, b) if (PART == BWD_SIGMA && threadIdx.x == 0 && blockIdx.x < 512) ncn_sigma_times[blockIdx.x][i] += (b) - (a)
#define SG_TREAL(i) if (PART == BWD_SIGMA && threadIdx.x == 0 && blockIdx.x < 512) ncn_sigma_times[blockIdx.x][i] = __builtin_amdgcn_s_memrealtime()
#define SG_TWAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define SG_TNOW(v)
#define SG_TADD(i, a, b)
#define SG_TREAL(i)
#define SG_TWAIT()
#endif

// The scatter (tools/scatter_probe.py): NCN_DIAG_SC_TIMES records wave 0's cycles per phase of
// the fine-level units; NCN_DIAG_SC_LEVELS_MASK skips the levels whose bit is clear (sc_one_unit).
#ifdef NCN_DIAG_SC_SPAN
__device__ unsigned long long ncn_sc_span[256][20];  // per workgroup: realtime (100 MHz) start/end, cycles start/end,
                                                     // then (unit, realtime at its end) for the first 8 units
#endif
#ifdef NCN_DIAG_SC_TIMES
__device__ unsigned long long ncn_sc_times[256][10];  // per workgroup, wave 0: cycles per phase
#define SC_TNOW(v) const unsigned long long v = __builtin_readcyclecounter()
#define SC_TADD(i, a, b) if (threadIdx.x == 0 && blockIdx.x < 256) ncn_sc_times[blockIdx.x][(i) * 2 + 1] += (b) - (a)
#define SC_TADDC(i, a, b) if (threadIdx.x == 0 && blockIdx.x < 256) ncn_sc_times[blockIdx.x][(i) * 2] += (b) - (a)
#define SC_TWAIT() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#else
#define SC_TNOW(v)
#define SC_TADD(i, a, b)
#define SC_TADDC(i, a, b)
#define SC_TWAIT()
#endif
}  // namespace ncn
extern "C" {
#ifdef NCN_DIAG_SC_TIMES
int ncn_diag_sc_times(unsigned long long* host, int reset) {
    if (reset) {
        static unsigned long long zero[256][10];
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(ncn::ncn_sc_times), zero, sizeof(zero));
    }
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(ncn::ncn_sc_times), 256 * 10 * sizeof(unsigned long long));
}
#endif
#ifdef NCN_DIAG_SIGMA_TIMES
int ncn_diag_sigma_times(unsigned long long* host, int reset) {
    if (reset) {
        static unsigned long long zero[512][10];
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(ncn::ncn_sigma_times), zero, sizeof(zero));
    }
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(ncn::ncn_sigma_times), 512 * 10 * sizeof(unsigned long long));
}
#endif
#ifdef NCN_DIAG_SC_SPAN
int ncn_diag_sc_span(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(ncn::ncn_sc_span), 256 * 20 * sizeof(unsigned long long));
}
#endif
}  // extern "C"
