// natgrad_dev.h — what the natural-gradient units share (natgrad.hip, natgrad_conv.hip): the padded
// sizes, the 32x32x2 f32 MFMA tile, the fixed-order sums, the layout of a gradient G = [dW ; db]
// and the table checks. Every unit gets its own copy (unnamed namespace).
#pragma once
#include "kf_common.h"
#include "../../include/kf_ops.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;        // init, trx, apply: 4 waves
constexpr int kMaxR = KF_NG_MAX_RANK;
constexpr int kPChunk = 256;         // rows of G per partial product of pass 1
typedef float f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ inline int ng_rp(int R) { return (R + 31) / 32 * 32; }
__host__ __device__ inline int ng_up32(int n) { return (n + 31) / 32 * 32; }
__host__ __device__ inline int ng_ldh(int D) { return KF_NG_W16_LD(D); }
inline size_t ng_align(size_t b) { return (b + 255) / 256 * 256; }

// 32x32x2 f32 MFMA: lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31];
// register g of lane l holds D[row (g & 3) + 8 (g >> 2) + 4 (l >> 5)][col l & 31]
__device__ __forceinline__ int ng_drow(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

// acc[i][j] = sum_{k < len} a(i, k) b(k, j) as one k-ordered chain; a(r, k) and b(k, r) are
// called with this lane's r and k < len only
template <class FA, class FB>
__device__ __forceinline__ f32x16 ng_tile(int len, FA a, FB b) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < len; k0 += 16) {  // rounds of 8 k steps, loads first
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + 2 * u + h;
            av[u] = k < len ? a(r, k) : 0.f;
            bv[u] = k < len ? b(k, r) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    }
    return acc;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}
// the workgroup's sum in every thread: the wave by shuffles, the waves through LDS in wave order
__device__ __forceinline__ double block_sum_all(double x, double *sh, int nwaves) {
    x = wave_sum(x);
    __syncthreads();  // sh may still be read from the sum before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < nwaves; ++w) s += sh[w];
    return s;
}

__host__ __device__ inline int ng_din(const KfNgComp &c) { return c.K + (c.db_off >= 0 ? 1 : 0); }
__host__ __device__ inline int ng_colgroups(int N) { return (ng_up32(N) / 32 + 3) / 4; }
__host__ __device__ inline int ng_pchunks(int din) { return (din + kPChunk - 1) / kPChunk; }
// element (row, col) of G = [dW ; db]
__device__ __forceinline__ long long ng_gidx(const KfNgComp &c, int row, int col) {
    return row < c.K ? c.dw_off + (long long)row * c.N + col : c.db_off + col;
}

bool ng_check_pres(const KfNgPre *pres, int npre, const char *who) {
    if (npre < 0 || (npre > 0 && !pres)) {
        kf_report_error("%s: bad preconditioner table (%d entries)", who, npre);
        return false;
    }
    for (int m = 0; m < npre; ++m) {
        const KfNgPre &p = pres[m];
        if (p.R < 8 || p.R > kMaxR || p.D <= p.R || p.w_off < 0 || p.h_off < 0 || p.s_off < 0 || p.st_off < 0) {
            kf_report_error("%s: preconditioner %d has dimension %d and rank %d; 8 <= rank <= %d, rank < dimension "
                            "and offsets >= 0 are required", who, m, p.D, p.R, kMaxR);
            return false;
        }
    }
    return true;
}

bool ng_check_opts(const KfNgOpts *o, const char *who) {
    if (!o || !(o->num_samples_history > 0.f) || !(o->alpha >= 0.f) || !(o->epsilon > 0.f) || !(o->delta >= 0.f) ||
        o->update_period < 1) {
        kf_report_error("%s: bad options", who);
        return false;
    }
    return true;
}

int ng_launched(const char *who) {
    return hipGetLastError() == hipSuccess ? 0 : (kf_report_error("%s: launch failed", who), -1);
}

}  // namespace
