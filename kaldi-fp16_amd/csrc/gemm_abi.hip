// gemm_abi.hip — the small row kernels of kf_ops.h (kf_rows_sum, kf_rows_sum_mask,
// kf_dot2_rows) and the reference ABI's GEMM (ops.h: ops_gemm through kf_ops_gemm_impl): the
// fused MFMA product where the operands allow it, scalar and short-K kernels elsewhere.
#include "gemm_host.h"
#include "../../include/ops.h"

__global__ void k_rows_sum(h16 *edge, const h16 *src, long long ld, int r0, int r1, int cols,
                           const uint8_t *mask) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int r = r0; r < r1; ++r) {
        const long long i = (long long)r * ld + c;
        if (!mask || ((mask[i >> 3] >> (i & 7)) & 1u)) s += h2f(src[i]);
    }
    edge[c] = f2h(s);
}

extern "C" int kf_rows_sum_mask(void *edge, const void *src, long long ld, int r0, int r1, int cols,
                                const uint8_t *mask) {
    kf_take_pending(__func__);
    if (cols <= 0) return 0;
    k_rows_sum<<<(cols + 255) / 256, 256, 0, kf_stream()>>>((h16 *)edge, (const h16 *)src, ld,
                                                            r0, r1, cols, mask);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kf_report_error("rows_sum: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}
extern "C" int kf_rows_sum(void *edge, const void *src, long long ld, int r0, int r1, int cols) {
    return kf_rows_sum_mask(edge, src, ld, r0, r1, cols, nullptr);
}

// out[j] = rne_fp16(x0 . W[j] + x1 . W[rows + j]) for j < rows (W [2*rows x cols], fp32
// accumulation): one row of a two-part product, e.g. the clamped-edge row T-1 of the MXFP8
// affine input gradient (network.cpp). A workgroup per output element: a one-row GEMM would
// walk K on two workgroups.
__global__ __launch_bounds__(256) void k_dot2_rows(h16 *out, const h16 *x0, const h16 *x1, const h16 *W, int rows,
                                                   int cols) {
    __shared__ float part[4];
    const int j = blockIdx.x;
    const h16 *w0 = W + (long long)j * cols, *w1 = W + (long long)(rows + j) * cols;
    float acc = 0.f;
    for (int c = 8 * threadIdx.x; c < cols; c += 8 * blockDim.x) {
        const half8 a = load_h8(x0 + c), b = load_h8(x1 + c), u = load_h8(w0 + c), v = load_h8(w1 + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf((float)a[e], (float)u[e], fmaf((float)b[e], (float)v[e], acc));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[j] = f2h(part[0] + part[1] + part[2] + part[3]);
}

extern "C" int kf_dot2_rows(void *out, const void *x0, const void *x1, const void *W, int rows, int cols) {
    kf_take_pending(__func__);
    if (rows <= 0) return 0;
    if (cols % 8 || ((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)W) & 15) {
        kf_report_error("kf_dot2_rows: cols %% 8 and 16-byte aligned operands required (cols=%d)", cols);
        return -1;
    }
    k_dot2_rows<<<rows, 256, 0, kf_stream()>>>((h16 *)out, (const h16 *)x0, (const h16 *)x1, (const h16 *)W, rows,
                                              cols);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kf_report_error("kf_dot2_rows: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// reference ABI GEMM (ops.h) on the fused product's kernels
// ---------------------------------------------------------------------------
struct KfGemmCtx {
    int magic;
};

extern "C" void *ops_cublas_create(void) {
    KfGemmCtx *c = new KfGemmCtx;
    c->magic = 0x6b663136;
    return c;
}
extern "C" void ops_cublas_destroy(void *h) { delete (KfGemmCtx *)h; }

// scalar fallback for shapes the MFMA path cannot address (unaligned / odd N)
__global__ void k_gemm_small(int M, int N, int K, float alpha, const h16 *A, int lda,
                             const h16 *B, int ldb, float beta, h16 *C, int ldc) {
    const long long total = (long long)M * N;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(i / N), n = (int)(i - (long long)m * N);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += h2f(A[(long long)m * lda + k]) * h2f(B[(long long)k * ldb + n]);
        float v = alpha * s;
        if (beta != 0.f) v += beta * h2f(C[(long long)m * ldc + n]);
        C[(long long)m * ldc + n] = f2h(v);
    }
}

// short-K products on 8-column vectors (K <= 8: AddBias is ops_gemm with K = 1 against a
// ones column, internal/gpu/ops.go:335-351): a thread owns one 8-column vector of C for
// all its rows and keeps B's K x 8 block in registers; A's K values of a row are the same
// for every thread of that row (one cached line). Same arithmetic and order as
// k_gemm_small: s = sum_k a*b in fp32, v = alpha * s (+ beta * C), one RNE store.
constexpr int kSmallK = 8;
template <int KS>
__global__ __launch_bounds__(256) void k_gemm_smallk_v8(int M, int ncv, int K, long long R, float alpha,
                                                        const h16 *A, int lda, const h16 *B, int ldb,
                                                        float beta, h16 *C, int ldc) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)ncv * R) return;
    const int cv = (int)(g % ncv);
    float b[KS][8];
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        if (k < K) {
            const half8 v = *reinterpret_cast<const half8 *>(B + (long long)k * ldb + 8 * cv);
#pragma unroll
            for (int e = 0; e < 8; ++e) b[k][e] = (float)v[e];
        }
    }
    // four rows in flight per thread (AddBias: K = 1, C's rows are the HBM stream). Every
    // load of a group is issued before its first store: vmcnt also counts stores, so a load
    // issued behind a store would wait for that store's acknowledgement.
    auto row = [&](long long m, const float (&a)[KS], const half8 &c0) {
        half8 out;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < KS; ++k)
                if (k < K) s += a[k] * b[k][e];
            float v = alpha * s;
            if (beta != 0.f) v += beta * (float)c0[e];
            out[e] = f2h(v);
        }
        *reinterpret_cast<half8 *>(C + m * ldc + 8 * cv) = out;
    };
    auto load = [&](long long m, float (&a)[KS], half8 &c0) {
#pragma unroll
        for (int k = 0; k < KS; ++k) a[k] = k < K ? h2f(A[m * lda + k]) : 0.f;
        c0 = beta != 0.f ? *reinterpret_cast<const half8 *>(C + m * ldc + 8 * cv) : half8{};
    };
    long long m = g / ncv;
    for (; m + 3 * R < M; m += 4 * R) {
        float a[4][KS];
        half8 c0[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) load(m + u * R, a[u], c0[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) row(m + u * R, a[u], c0[u]);
    }
    for (; m < M; m += R) {
        float a[KS];
        half8 c0;
        load(m, a, c0);
        row(m, a, c0);
    }
}

int kf_ops_gemm_impl(int M, int N, int K, float alpha, const void *A, int lda, const void *B,
                     int ldb, float beta, void *C, int ldc, char *err, size_t errlen) {
    kf_take_pending(__func__);
    if (M < 0 || N < 0 || K < 0) {
        snprintf(err, errlen, "ops_gemm: negative dims (M=%d N=%d K=%d)", M, N, K);
        return -1;
    }
    if (M == 0 || N == 0) return 0;
    if (lda <= 0) lda = K;
    if (ldb <= 0) ldb = N;
    if (ldc <= 0) ldc = N;
    const bool fast = (K % 8 == 0) && (N % 8 == 0) && (lda % 8 == 0) && (ldb % 8 == 0) &&
                      (ldc % 8 == 0) && !(((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15);
    const bool smallk_vec = K <= kSmallK && N % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 &&
                            !(((uintptr_t)B | (uintptr_t)C) & 15);
    if (smallk_vec) {
        const int ncv = N / 8;
        long long R = 524288 / ncv;
        if (R < 1) R = 1;
        if (R > M) R = M;
        const unsigned grid = (unsigned)((ncv * R + 255) / 256);
        if (K == 1)  // AddBias (ops.go:335-351): one column of B in registers
            k_gemm_smallk_v8<1><<<grid, 256, 0, kf_stream()>>>(M, ncv, K, R, alpha, (const h16 *)A, lda,
                                                                (const h16 *)B, ldb, beta, (h16 *)C, ldc);
        else
            k_gemm_smallk_v8<kSmallK><<<grid, 256, 0, kf_stream()>>>(M, ncv, K, R, alpha, (const h16 *)A, lda,
                                                                      (const h16 *)B, ldb, beta, (h16 *)C, ldc);
    } else if (!fast || K == 0) {
        k_gemm_small<<<kf_blocks((long long)M * N, 256, 8192), 256, 0, kf_stream()>>>(
            M, N, K, alpha, (const h16 *)A, lda, (const h16 *)B, ldb, beta, (h16 *)C, ldc);
    } else {
        KfOperand a = plain_operand(A, lda, M, K, 1);
        KfOperand b = plain_operand(B, ldb, K, N, 0);
        KfEpilogue E;
        memset(&E, 0, sizeof(E));
        E.out = C;
        E.ldo = ldc;
        E.alpha = alpha;
        E.beta = beta;
        if (kf_gemm_fused(M, N, K, &a, &b, &E) != 0) {
            snprintf(err, errlen, "%s", kf_last_error() ? kf_last_error() : "gemm failed");
            return -1;
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(err, errlen, "ops_gemm (M=%d N=%d K=%d): %s", M, N, K, hipGetErrorString(e));
        return -1;
    }
    return 0;
}
