// update.hip — the Kaldi-style parameter update over the flat parameter set
// (include/kf_ops.h kf_update_maxchange): momentum SGD with a
// per-component L2 term and learning-rate factor, each component's step limited to its
// max-change and the whole step to max_param_change.
//
// Three launches on the current stream, no host round trip, no atomics:
//   k_upd_velocity  v <- mom*v + g + l2*w, and per workgroup the sum of d^2, d = lr*lrf*v
//   k_upd_scales    per component n_c and s_c, then N and S: one workgroup
//   k_upd_apply     w32 <- w32 - S*s_c*d, w16 <- rne(w32)
// A workgroup owns one chunk of KF_UPD_CHUNK elements of one segment, so it never mixes two
// components; the chunk is found by a search over the segments' first_wg. All three are
// HBM-bound (16 + 14 bytes per parameter); the body moves 16-byte vectors.
//
// Every sum runs in a fixed order (per thread in address order, the wave by shuffles, the
// waves through LDS in wave order, the workgroups' partials lane-strided in double and the
// same shuffle tree), so two runs on the same inputs give the same bits.
//
// kf_update_maxchange_scaled is the same three launches with the dynamic loss
// scale's state: each kernel's LS instantiation loads skip and inv_used block-uniformly, returns
// before it has written a byte on skip and reads g * inv_used otherwise. The plain call runs the
// LS = false instantiations, which are the kernels as they were.
#include "upd_chunk.h"

namespace {

constexpr int kThreads = 256;
constexpr int kScaleThreads = 1024;  // k_upd_scales: 16 waves, each a component at a time
static_assert(KF_UPD_CHUNK % (4 * kThreads) == 0, "a chunk is whole float4 rounds of the workgroup");

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}

// v = mom*v + g + l2s*w, rounded once: the three terms are summed in double (the kernel is
// HBM-bound, the fp64 rate is not in its way), so a cancellation between them costs no bits
__device__ __forceinline__ float upd_velocity(float mom, float v, float g, double l2s, float w) {
    return (float)((double)mom * (double)v + (double)g + l2s * (double)w);
}

// the gradient a scaled update reads: g / (the scale it was made with). The barrier keeps the
// product out of any contraction with what follows, so the rest is the plain kernel's arithmetic
__device__ __forceinline__ float upd_unscale(float g, float inv) {
    float r = g * inv;
    asm volatile("" : "+v"(r));
    return r;
}

template <bool LS>
__global__ __launch_bounds__(kThreads) void k_upd_velocity(const float *__restrict__ w32, const float *__restrict__ g,
                                                           float *__restrict__ v, long long n,
                                                           const KfUpdSegment *__restrict__ segs, int nseg,
                                                           const KfUpdComp *__restrict__ comps, int ncomp, float lr, float mom,
                                                           float l2_scale, float *__restrict__ partial,
                                                           const KfLossScaleState *__restrict__ ls) {
    float inv = 1.f;
    if constexpr (LS) {
        if (ls->skip) return;  // block-uniform: nothing of v is written
        inv = ls->inv_used;
    }
    long long cb, ce, a0, a1;
    int c;
    if (!upd_chunk(segs, nseg, ncomp, n, blockIdx.x, cb, ce, c)) return;  // the same in every thread
    const KfUpdComp cp = comps[c];
    const double l2s = (double)l2_scale * (double)cp.l2;
    const bool l2on = l2s != 0.0;  // without an L2 term the weights are not read
    const float dl = lr * cp.lr_factor;
    upd_split(cb, ce, a0, a1);
    float acc = 0.f;
    for (long long i = a0 + 4 * threadIdx.x; i < a1; i += 4 * kThreads) {
        float4v gv = *reinterpret_cast<const float4v *>(g + i);
        float4v vv = *reinterpret_cast<const float4v *>(v + i);
        float4v wv = {0.f, 0.f, 0.f, 0.f};
        if (l2on) wv = *reinterpret_cast<const float4v *>(w32 + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (LS) gv[e] = upd_unscale(gv[e], inv);
            vv[e] = upd_velocity(mom, vv[e], gv[e], l2s, wv[e]);
            const float d = dl * vv[e];
            acc += d * d;
        }
        *reinterpret_cast<float4v *>(v + i) = vv;
    }
    const long long i = upd_scalar(cb, ce, a0, a1, threadIdx.x);
    if (i >= 0) {
        const float gi = LS ? upd_unscale(g[i], inv) : g[i];
        const float vn = upd_velocity(mom, v[i], gi, l2s, l2on ? w32[i] : 0.f);
        v[i] = vn;
        const float d = dl * vn;
        acc += d * d;
    }
    __shared__ float sh[kThreads / 64];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = sh[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) s += sh[w];
        partial[blockIdx.x] = s;
    }
}

// One workgroup. Wave w takes components w, w + 16, ...: its lanes sum the component's
// workgroup partials lane-strided in double, then the shuffle tree. n_c, s_c -> stats,
// (s_c n_c)^2 -> clip2; then wave 0 sums clip2 the same way for N and S, and every thread
// writes step[c] = S * s_c * lr * lrf_c, the factor k_upd_apply multiplies v by.
// LS, on skip: the partials were not written; the report is all zero (n_c, s_c, N, S) and so is step.
template <bool LS>
__global__ __launch_bounds__(kScaleThreads) void k_upd_scales(const KfUpdComp *__restrict__ comps, int ncomp,
                                                         const float *__restrict__ partial, int npartial, float lr,
                                                         float max_param_change, double *__restrict__ clip2,
                                                         float *__restrict__ step, float *__restrict__ stats,
                                                         const KfLossScaleState *__restrict__ ls) {
    if constexpr (LS) {
        if (ls->skip) {
            for (int i = threadIdx.x; i < 2 * ncomp + 2; i += kScaleThreads) stats[i] = 0.f;
            for (int c = threadIdx.x; c < ncomp; c += kScaleThreads) step[c] = 0.f;
            return;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < ncomp; c += kScaleThreads / 64) {
        const KfUpdComp cp = comps[c];
        int p0 = cp.first_wg < 0 ? 0 : cp.first_wg;
        int p1 = cp.first_wg + cp.num_wg;
        if (p1 > npartial) p1 = npartial;
        double s = 0.0;
        for (int p = p0 + lane; p < p1; p += 64) s += (double)partial[p];
        s = wave_sum(s);
        if (lane == 0) {
            const double nc = sqrt(s);
            const double sc = (cp.max_change > 0.f && nc > (double)cp.max_change) ? (double)cp.max_change / nc : 1.0;
            stats[c] = (float)nc;
            stats[ncomp + c] = (float)sc;
            clip2[c] = (sc * nc) * (sc * nc);
        }
    }
    __syncthreads();  // clip2 and stats of every component are written (one workgroup)
    __shared__ double shS;
    if (wave == 0) {
        double s = 0.0;
        for (int c = lane; c < ncomp; c += 64) s += clip2[c];
        s = wave_sum(s);
        if (lane == 0) {
            const double N = sqrt(s);
            const double S = (max_param_change > 0.f && N > (double)max_param_change) ? (double)max_param_change / N : 1.0;
            stats[2 * ncomp] = (float)N;
            stats[2 * ncomp + 1] = (float)S;
            shS = S;
        }
    }
    __syncthreads();
    const double S = shS;
    for (int c = threadIdx.x; c < ncomp; c += kScaleThreads)
        step[c] = (float)(S * (double)stats[ncomp + c] * (double)lr * (double)comps[c].lr_factor);
}

// w16 = rne(the stored fp32 w): the barrier keeps hipcc from folding the update into
// v_fma_mixlo_f16, which rounds the exact w - f*v to fp16 once and differs from rne(w32) at
// near-ties (as in k_sgd_flat)
__device__ __forceinline__ float upd_weight(float w, float f, float v) {
    float r = w - f * v;
    asm volatile("" : "+v"(r));
    return r;
}

template <bool LS>
__global__ __launch_bounds__(kThreads) void k_upd_apply(float *__restrict__ w32, h16 *__restrict__ w16,
                                                        const float *__restrict__ v, long long n,
                                                        const KfUpdSegment *__restrict__ segs, int nseg, int ncomp,
                                                        const float *__restrict__ step,
                                                        const KfLossScaleState *__restrict__ ls) {
    if constexpr (LS) {
        if (ls->skip) return;  // block-uniform: nothing of w32 / w16 is written
    }
    long long cb, ce, a0, a1;
    int c;
    if (!upd_chunk(segs, nseg, ncomp, n, blockIdx.x, cb, ce, c)) return;
    const float f = step[c];
    upd_split(cb, ce, a0, a1);
    for (long long i = a0 + 4 * threadIdx.x; i < a1; i += 4 * kThreads) {
        const float4v vv = *reinterpret_cast<const float4v *>(v + i);
        float4v wv = *reinterpret_cast<const float4v *>(w32 + i);
        half4 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            wv[e] = upd_weight(wv[e], f, vv[e]);
            hv[e] = f2h(wv[e]);
        }
        *reinterpret_cast<float4v *>(w32 + i) = wv;
        *reinterpret_cast<half4 *>(w16 + i) = hv;
    }
    const long long i = upd_scalar(cb, ce, a0, a1, threadIdx.x);
    if (i >= 0) {
        const float w = upd_weight(w32[i], f, v[i]);
        w32[i] = w;
        w16[i] = f2h(w);
    }
}

size_t upd_align(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" long long kf_update_scratch_bytes(long long n, int nseg, int ncomp) {
    if (n < 0 || nseg < 0 || ncomp < 0) return -1;
    return (long long)(upd_align((size_t)upd_grid(n, nseg) * 4) + upd_align((size_t)ncomp * 8) +
                       upd_align((size_t)ncomp * 4));
}

static int update_maxchange(const char *fn, float *w32, void *w16, const float *g, float *v, long long n,
                            const KfUpdSegment *segments, int nseg, const KfUpdComp *comps, int ncomp, float lr,
                            float momentum, float max_param_change, float l2_scale, void *scratch, float *stats,
                            const KfLossScaleState *ls) {
    kf_take_pending(fn);
    if (n < 0 || nseg < 0 || ncomp < 0 || !(max_param_change >= 0.f)) {
        kf_report_error("%s: bad arguments (n %lld, %d segments, %d components, max_param_change %g)", fn, n, nseg, ncomp,
                        (double)max_param_change);
        return -1;
    }
    if (n == 0 || nseg == 0 || ncomp == 0) return 0;
    const long long grid = upd_grid(n, nseg);
    if (!w32 || !w16 || !g || !v || !segments || !comps || !scratch || !stats || grid > 0x7fffffffll ||
        ((uintptr_t)w32 | (uintptr_t)g | (uintptr_t)v) % 16 || (uintptr_t)w16 % 8 || (uintptr_t)scratch % 8 ||
        (uintptr_t)ls % 8) {
        kf_report_error("%s: null or misaligned buffer (w32 / g / v 16 bytes, w16 and scratch 8), or "
                        "more than 2^31 workgroups", fn);
        return -1;
    }
    float *partial = (float *)scratch;
    double *clip2 = (double *)((char *)scratch + upd_align((size_t)grid * 4));
    float *step = (float *)((char *)clip2 + upd_align((size_t)ncomp * 8));
    hipStream_t st = kf_stream();
    if (ls) {
        k_upd_velocity<true><<<(unsigned)grid, kThreads, 0, st>>>(w32, g, v, n, segments, nseg, comps, ncomp, lr, momentum,
                                                                  l2_scale, partial, ls);
        k_upd_scales<true><<<1, kScaleThreads, 0, st>>>(comps, ncomp, partial, (int)grid, lr, max_param_change, clip2, step,
                                                        stats, ls);
        k_upd_apply<true><<<(unsigned)grid, kThreads, 0, st>>>(w32, (h16 *)w16, v, n, segments, nseg, ncomp, step, ls);
    } else {
        k_upd_velocity<false><<<(unsigned)grid, kThreads, 0, st>>>(w32, g, v, n, segments, nseg, comps, ncomp, lr, momentum,
                                                                   l2_scale, partial, nullptr);
        k_upd_scales<false><<<1, kScaleThreads, 0, st>>>(comps, ncomp, partial, (int)grid, lr, max_param_change, clip2, step,
                                                         stats, nullptr);
        k_upd_apply<false><<<(unsigned)grid, kThreads, 0, st>>>(w32, (h16 *)w16, v, n, segments, nseg, ncomp, step, nullptr);
    }
    if (hipGetLastError() == hipSuccess) return 0;
    kf_report_error("%s: launch failed", fn);
    return -1;
}

extern "C" int kf_update_maxchange(float *w32, void *w16, const float *g, float *v, long long n,
                                   const KfUpdSegment *segments, int nseg, const KfUpdComp *comps, int ncomp, float lr,
                                   float momentum, float max_param_change, float l2_scale, void *scratch,
                                   float *stats) {
    return update_maxchange(__func__, w32, w16, g, v, n, segments, nseg, comps, ncomp, lr, momentum, max_param_change,
                            l2_scale, scratch, stats, nullptr);
}

extern "C" int kf_update_maxchange_scaled(float *w32, void *w16, const float *g, float *v, long long n,
                                          const KfUpdSegment *segments, int nseg, const KfUpdComp *comps, int ncomp,
                                          float lr, float momentum, float max_param_change, float l2_scale,
                                          void *scratch, float *stats, const void *loss_scale_state) {
    return update_maxchange(__func__, w32, w16, g, v, n, segments, nseg, comps, ncomp, lr, momentum, max_param_change,
                            l2_scale, scratch, stats, (const KfLossScaleState *)loss_scale_state);
}
