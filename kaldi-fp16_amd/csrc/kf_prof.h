// kf_prof.h — per-launch HIP-event timing (kf_prof_*, include/kf_ops.h) as the kernels'
// launch sites see it: the record classes, the generic bracket for launch sequences and the
// one timed launch of a single kernel. The records and the event pool are private to prof.hip.
#pragma once
#include <hip/hip_ext.h>

#include <type_traits>

#include "kf_common.h"

// record classes (kf_ops.h: kf_prof_collect)
enum {
    KF_PROF_FUSED = 0,       // fused GEMM
    KF_PROF_WGRAD = 1,       // weight-gradient GEMM
    KF_PROF_CHAIN_NUM = 2,   // chain numerator
    KF_PROF_CHAIN_DEN = 3,   // chain denominator
    KF_PROF_HALO = 4,        // conv halo forward / input gradient
    KF_PROF_HALO_WGRAD = 5,  // conv halo weight gradient
    KF_PROF_REDUCE = 6,      // split-K slab reduce
    KF_PROF_CHAIN_XENT = 7,  // chain xent derivative (kf_chain_xent)
};

// bracket of any launch sequence on the current stream (two event records): returns a
// record index for kf_prof_stop, or -1 when profiling is off
int kf_prof_start(int cls, double work);
int kf_prof_start2(int cls, double flops, double bytes);
void kf_prof_stop(int idx);

// what a launch site knows about one kernel launch
struct KfProfRec {
    int cls;
    double flops;
    double bytes;  // algorithmic HBM bytes: unique operand sources + epilogue reads / writes
    int m, n, k;   // GEMM shape (0 when not a GEMM)
    int tile;      // BM * 10000 + BN, or 0
};

#pragma GCC visibility push(hidden)
// profiling on: appends `rec` and hands out its two pooled events; off: returns false
bool kf_prof_take(const KfProfRec &rec, hipEvent_t *start, hipEvent_t *stop);
#pragma GCC visibility pop

// One kernel launch on kf_stream(), timed when `rec` is given and profiling is on. The
// dispatch packet itself then carries the start / stop timestamps: no marker packets
// between kernels (event records cost ~1 ms per step of gaps). rec == nullptr: untimed.
// (common_type_t: not deduced, so the arguments convert to the kernel's parameter types)
template <typename... KA>
static inline void kf_launch(void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds, const KfProfRec *rec,
                             std::common_type_t<KA>... args) {
    hipEvent_t a, b;
    if (rec && kf_prof_take(*rec, &a, &b))
        hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)lds, kf_stream(), a, b, 0, args...);
    else
        kernel<<<grid, block, lds, kf_stream()>>>(args...);
}
