// gemm_wgrad.hip — kf_gemm_wgrad / kf_gemm_wgrad_scaled (kf_ops.h): dW = X^T . dZ as a split-K
// gemm_kernel launch into fp32 slabs (both operands reduction-major) plus the slab reduce,
// which conv_wgrad.hip's halo kernel shares.
#include "gemm_kernel.h"

// split-K reduction: dst[m][n] (+)= sum_s slab[s][m][n], summed in split order (the
// result does not depend on the launch shape). Each thread owns 4 consecutive columns
// and keeps 8 slab loads in flight; the scalar form (one dependent load chain per
// element) ran at ~1.2 TB/s.
__device__ __forceinline__ void slab_reduce_body(const float *slab, int splits, int M, int N, float *dst,
                                                 long long ldw, int accumulate, int bid, int nblk,
                                                 const float *cs) {
    const long long total = (long long)M * N;
    const long long step = (long long)nblk * blockDim.x;
    if ((N & 3) == 0) {
        const long long t4 = total >> 2;
        const float4v *s4 = reinterpret_cast<const float4v *>(slab);
        for (long long i = (long long)bid * blockDim.x + threadIdx.x; i < t4; i += step) {
            float4v acc = {0.f, 0.f, 0.f, 0.f};
            int k = 0;
            for (; k + 8 <= splits; k += 8) {
                float4v v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(s4 + (k + u) * t4 + i);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
            }
            for (; k < splits; ++k) acc += __builtin_nontemporal_load(s4 + k * t4 + i);
            const long long e = 4 * i, m = e / N, n = e - m * N;
            float *d = dst + m * ldw + n;
            if (cs) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] *= cs[n + u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) d[u] = accumulate ? d[u] + acc[u] : acc[u];
        }
        return;
    }
    for (long long i = (long long)bid * blockDim.x + threadIdx.x; i < total; i += step) {
        float s = 0.f;
        for (int k = 0; k < splits; ++k) s += slab[k * total + i];
        const long long m = i / N, n = i - m * N;
        if (cs) s *= cs[n];
        float *d = dst + m * ldw + n;
        *d = accumulate ? *d + s : s;
    }
}

// bias column sums over the splits: 4 waves split the slabs of 64 columns, fixed-order
// combine (the one-thread-per-column form was latency bound: 27 us for 86 splits)
__device__ __forceinline__ void slab_reduce_cols_body(const float *slab, int splits, int N, float *dst,
                                                      int accumulate, int bid, const float *cs) {
    __shared__ float part[4][64];
    const int c = bid * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    float s = 0.f;
    if (c < N)
        for (int k = g; k < splits; k += 4) s += slab[(long long)k * N + c];
    part[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && c < N) {
        const int l = threadIdx.x & 63;
        float t = (part[0][l] + part[1][l]) + (part[2][l] + part[3][l]);
        if (cs) t *= cs[c];
        dst[c] = accumulate ? dst[c] + t : t;
    }
}

__global__ __launch_bounds__(256) void k_slab_reduce(const float *slab, int splits, int M, int N,
                                                     float *dst, long long ldw, int accumulate,
                                                     const float *cs) {
    slab_reduce_body(slab, splits, M, N, dst, ldw, accumulate, blockIdx.x, gridDim.x, cs);
}
// both reduces in one launch: the first ncb blocks sum the bias columns, the rest the
// dW slabs (the column job alone is a few latency-bound blocks: 9.5 us per launch)
__global__ __launch_bounds__(256) void k_slab_reduce_both(const float *slab, int splits, int M, int N,
                                                          float *dst, long long ldw, int accumulate,
                                                          const float *bias_slab, float *bias_dst, int ncb,
                                                          const float *cs) {
    if ((int)blockIdx.x < ncb)
        slab_reduce_cols_body(bias_slab, splits, N, bias_dst, accumulate, blockIdx.x, cs);
    else
        slab_reduce_body(slab, splits, M, N, dst, ldw, accumulate, blockIdx.x - ncb, gridDim.x - ncb, cs);
}

// split-K reduce of kf_gemm_wgrad's slabs (also used by conv_wgrad.hip)
void kf_wgrad_reduce(const float *slab, const float *bias_slab, int splits, int M, int N, float *dW,
                     long long ldw, float *bias_grad, int accumulate, const float *cs) {
    const int nb = kf_blocks((long long)M * N / 4 + 1, 256, 4096);
    const int ncb = bias_grad ? (N + 63) / 64 : 0;
    KfProfRec rec{};
    rec.cls = KF_PROF_REDUCE;
    // the slabs read once, dW (and the bias) written once (+ read when accumulating)
    rec.bytes = ((double)splits * (M + (bias_grad ? 1 : 0)) + (accumulate ? 2.0 : 1.0) * (M + 1)) * N * 4.0;
    if (bias_grad)
        kf_launch(k_slab_reduce_both, dim3(ncb + nb), dim3(256), 0, &rec, slab, splits, M, N, dW, ldw, accumulate,
                  bias_slab, bias_grad, ncb, cs);
    else
        kf_launch(k_slab_reduce, dim3(nb), dim3(256), 0, &rec, slab, splits, M, N, dW, ldw, accumulate, cs);
}

// workgroups per weight-gradient launch (split-K target): 512 alone on the device; nnet's
// backward sets 256 while its weight gradients run on their own stream beside the
// input-gradient chain (half the CUs each, half the fp32 slab bytes)
static thread_local int g_wgrad_target = 512;
extern "C" int kf_gemm_wgrad_target(int wgs) {
    const int old = g_wgrad_target;
    if (wgs > 0) g_wgrad_target = wgs;
    return old;
}

static int wgrad_impl(int M, int N, int K, const KfOperand *A, const KfOperand *B, float *dW, long long ldw,
                      float *bias_grad, int accumulate, const float *cs) {
    kf_take_pending(__func__);
    if (M <= 0 || N <= 0) return 0;
    OpD a, b;
    if (!to_dev(*A, a, "A") || !to_dev(*B, b, "B")) return -1;
    if (b.tmul > 1 || b.t0) {
        kf_report_error("kf_gemm_wgrad: time-strided rows (tmul / t0) only on the conv im2col operand A");
        return -1;
    }
    if (A->kcontig || B->kcontig) {
        kf_report_error("kf_gemm_wgrad: A and B must be reduction-major");
        return -1;
    }
    if (!mn_gen_ok(a, "A") || !mn_gen_ok(b, "B")) return -1;
    if (a.mk || (b.mk && (op_mode(b) != OP_SIMPLE || op_mode(a) == OP_GEN))) {
        kf_report_error("kf_gemm_wgrad: a masked operand must be a plain B (A plain or a two-part time splice)");
        return -1;
    }
    // 3x3 convolutions: the source halo in LDS instead of nine im2col slabs
    if (!b.mk) {
        const int hr = kf_conv_wgrad_halo_try(M, N, K, a, b, dW, ldw, bias_grad, accumulate);
        if (hr != 0) return hr < 0 ? -1 : 0;
    }
    if (a.tmul > 1 || a.t0) {
        kf_report_error("kf_gemm_wgrad: time-strided rows (tmul / t0) need a 3x3 conv on the halo kernel");
        return -1;
    }
    // tiles: 384x160 for N = 160 / 320 (TDNN-F linear); otherwise 64-, 128- or 256-column
    // tiles whose row count (192, 256 or 320) wastes the fewest padded rows of M
    int BMc = 256, BNc = (N % 160 == 0 && N <= 320) ? 160 : N <= 64 ? 64 : N <= 128 ? 128 : 256;
    if (BNc == 160) {
        BMc = 384;
    } else {
        const int cands[3] = {256, BNc == 256 ? 320 : 256, 192};
        long long bw = (long long)(M + 255) / 256 * 256;
        for (int c : cands) {
            const long long w = (long long)(M + c - 1) / c * c;
            if (w < bw) bw = w, BMc = c;
        }
    }
    // (r5: two workgroups per CU for the TDNN-F weight gradients, 160x128 / 128x160 tiles at
    // 72 KB, a quarter of the fp32 slab bytes: affine 121 -> 311 us, linear 126 -> 171 us per
    // launch, the reduce 25 -> 13 us; the bigger tiles' operand reuse is worth more)
    const int tiles = ((M + BMc - 1) / BMc) * ((N + BNc - 1) / BNc);
    // workgroups per launch: every split writes an M x N fp32 slab that the reduce
    // reads back, so the target trades CU fill against slab traffic
    // (targets of 256 / 384 / 768 / 1024 measured slower)
    // at most the target (rounding the split count down): beside the input-gradient chain a
    // launch with a few workgroups more than fit at once holds them pending until a whole
    // workgroup's K range retires, and the chain's launches queue behind them (a 4-row
    // edge sum took 128 us instead of 6.5; bench 36.90-37.02 -> 36.57-36.65 ms, r5)
    int splits = std::max(1, g_wgrad_target / tiles);
    const int maxsplit = (K + 4 * BK - 1) / (4 * BK);  // at least 4 K-steps per split
    if (splits > maxsplit) splits = maxsplit;
    if (splits < 1) splits = 1;
    int kps = (K + splits - 1) / splits;
    kps = (kps + BK - 1) / BK * BK;
    splits = (K + kps - 1) / kps;
    size_t slab_bytes = (size_t)splits * M * N * 4;
    size_t bias_bytes = bias_grad ? (size_t)splits * N * 4 : 0;
    char *ws = (char *)kf_workspace_stream(slab_bytes + bias_bytes + 256);
    if (!ws) {
        kf_report_error("kf_gemm_wgrad: workspace allocation of %zu bytes failed",
                        slab_bytes + bias_bytes);
        return -1;
    }
    WgradArgs G{(float *)ws,
                bias_grad ? (float *)(ws + ((slab_bytes + 255) & ~(size_t)255)) : nullptr, kps, 0, 0};
    KfEpilogue E{};
    const int am = op_mode(a), bm = op_mode(b);
    // the TDNN-F linear's [x(t - s) | x(t)]: pair the parts' tiles per XCD
    if (am == OP_P2 && A->nparts == 2 && N <= BNc && A->part_width % BMc == 0 &&
        M == 2 * A->part_width)
        G.pair_ps = A->part_width / BMc;
    int rc;
#define KF_WG(AM_, BM_)                                                                          \
    do {                                                                                         \
        if (BMc == 320 && BNc == 256)                                                            \
            rc = launch<320, 256, 2, 4, false, false, true, 2, AM_, BM_>(M, N, K, a, b, E, G, splits); \
        else if (BMc == 192 && BNc == 256)                                                       \
            rc = launch<192, 256, 2, 4, false, false, true, 2, AM_, BM_>(M, N, K, a, b, E, G, splits); \
        else if (BMc == 192 && BNc == 128)                                                       \
            rc = launch<192, 128, 4, 2, false, false, true, 2, AM_, BM_>(M, N, K, a, b, E, G, splits); \
        else if (BMc == 192 && BNc == 64)                                                        \
            rc = launch<192, 64, 4, 1, false, false, true, 2, AM_, BM_>(M, N, K, a, b, E, G, splits); \
        else if (BMc == 256 && BNc == 256)                                                       \
            rc = launch<256, 256, 2, 4, false, false, true, 2, AM_, BM_>(M, N, K, a, b, E, G, splits); \
        else if (BMc == 256 && BNc == 128)                                                       \
            rc = launch<256, 128, 4, 2, false, false, true, 2, AM_, BM_>(M, N, K, a, b, E, G, splits); \
        else if (BNc == 160)                                                                     \
            rc = launch<384, 160, 4, 2, false, false, true, 2, AM_, BM_>(M, N, K, a, b, E, G, splits); \
        else                                                                                     \
            rc = launch<256, 64, 4, 1, false, false, true, 2, AM_, BM_>(M, N, K, a, b, E, G, splits); \
    } while (0)
    if (b.mk) {
        // masked B (the TDNN-F affine weight gradient on the implicit dz, N = layer width)
        if (BNc != 256) {
            kf_report_error("kf_gemm_wgrad: masked B needs N > 128 (M=%d N=%d)", M, N);
            return -1;
        }
#define KF_WGM(AM_)                                                                                      \
    do {                                                                                                 \
        if (BMc == 320)                                                                                  \
            rc = launch<320, 256, 2, 4, false, false, true, 2, AM_, OP_SIMPLE | OP_MASKED>(M, N, K, a, b, E, G, splits); \
        else if (BMc == 192)                                                                             \
            rc = launch<192, 256, 2, 4, false, false, true, 2, AM_, OP_SIMPLE | OP_MASKED>(M, N, K, a, b, E, G, splits); \
        else                                                                                             \
            rc = launch<256, 256, 2, 4, false, false, true, 2, AM_, OP_SIMPLE | OP_MASKED>(M, N, K, a, b, E, G, splits); \
    } while (0)
        if (am == OP_SIMPLE) KF_WGM(OP_SIMPLE);
        else KF_WGM(OP_P2);
#undef KF_WGM
    } else if (bm == OP_SIMPLE && am == OP_SIMPLE) KF_WG(OP_SIMPLE, OP_SIMPLE);
    else if (bm == OP_SIMPLE && am == OP_P2) KF_WG(OP_P2, OP_SIMPLE);
    else if (bm == OP_SIMPLE) KF_WG(OP_GEN, OP_SIMPLE);
    else KF_WG(OP_GEN, OP_GEN);
#undef KF_WG
    if (rc) return rc;
    kf_wgrad_reduce(G.slab, G.bias_slab, splits, M, N, dW, ldw, bias_grad, accumulate, cs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kf_report_error("wgrad reduce: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

extern "C" int kf_gemm_wgrad(int M, int N, int K, const KfOperand *A, const KfOperand *B,
                             float *dW, long long ldw, float *bias_grad, int accumulate) {
    return wgrad_impl(M, N, K, A, B, dW, ldw, bias_grad, accumulate, nullptr);
}
extern "C" int kf_gemm_wgrad_halo_applies(int M, int N, int K, const KfOperand *A, const KfOperand *B) {
    OpD a, b;
    if (!A || !B || !to_dev(*A, a, "A") || !to_dev(*B, b, "B")) return -1;
    return !b.mk && kf_conv_wgrad_halo_applies(M, N, K, a, b) ? 1 : 0;
}
extern "C" int kf_gemm_wgrad_scaled(int M, int N, int K, const KfOperand *A, const KfOperand *B, float *dW,
                                    long long ldw, float *bias_grad, int accumulate, const float *col_scale) {
    if (!col_scale) {
        kf_report_error("kf_gemm_wgrad_scaled: null col_scale");
        return -1;
    }
    return wgrad_impl(M, N, K, A, B, dW, ldw, bias_grad, accumulate, col_scale);
}
