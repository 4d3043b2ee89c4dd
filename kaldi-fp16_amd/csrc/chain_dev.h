// chain_dev.h — what the chain objective's units share: the log-domain and reduction
// device helpers of the numerator and denominator kernels, the numerator descriptor
// LogFstDev (k_den_post reads it in product mode), and two small host helpers for device
// memory.
#pragma once
#include "kf_common.h"

#include <algorithm>
#include <vector>

static const float kLogZero = -1.0e+30f;
static const float kFix = 17592186044416.0f;          // 2^44
static const double kInvFix = 1.0 / 17592186044416.0;  // 2^-44

// ===========================================================================
// Device helpers
// ===========================================================================
__device__ __forceinline__ float logadd_dev(float a, float b) {  // chain_det.cu:26-35
    if (a <= kLogZero) return b;
    if (b <= kLogZero) return a;
    float mx = fmaxf(a, b), mn = fminf(a, b);
    return mx + log1pf(expf(mn - mx));
}

template <typename XT>
__device__ __forceinline__ float ld_x(const XT *p) { return (float)*p; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Deterministic block sum: wave butterflies, then the per-wave sums in wave order.
// Every thread returns the same value. Contains one barrier; `red` must not be
// reused before the next barrier.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    return s;
}
template <int NW>
__device__ __forceinline__ double block_sum_d(double v, double *red) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    return s;
}

// ===========================================================================
// Descriptor of one numerator FST and its run (chain_num.hip's kernels)
// ===========================================================================
struct LogFstDev {
    const int *row_ptr, *in_ptr, *in_arc, *arc_src, *arc_dst, *arc_pdf;
    const float *arc_w;
    const int *grp_ptr, *grp_pdf, *grp_arc;
    // pre-gathered copies for the LDS-resident kernel (k_num_fb)
    const int *in_src, *in_g, *arc_g, *gsrc, *gdst;
    const float *in_w, *gw;
    const int *fin_state;
    const float *fin_w;
    int S, A, G, nfinal, start, T;
    int mode;        // bit0: forward+backward, bit1: posteriors
    int stride;
    long long row0;  // frame t -> nnet row row0 + t*stride
    float *alpha, *beta;  // [(T+1) x S]
    float *post_sparse;   // [T x G] or null
    float *post_dense;    // [T x P] or null
    float *total;         // [1] (in: when mode has no forward)
};

enum { LF_FB = 1, LF_POST = 2 };

// ===========================================================================
// Host: device memory helpers
// ===========================================================================
#pragma GCC visibility push(hidden)  // internal to libkaldi_fp16.so

template <typename T>
T *dev_upload(const std::vector<T> &v, std::vector<void *> &owned) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    owned.push_back(p);
    if (!v.empty()) hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return (T *)p;
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) hipFree(p);
    }
    bool alloc(size_t n) {
        return hipMalloc(&p, std::max<size_t>(n, 16)) == hipSuccess;
    }
};

#pragma GCC visibility pop
