// quant_mxfp8.hip — MXFP8 quantisation of fp16 matrices (kf_ops.h: kf_quant_mxfp8,
// kf_quant_mxfp8_batch): e4m3 payload, one E8M0 scale per 32 elements of a row.
#include "gemm_common.h"

// ---------------------------------------------------------------------------
// MXFP8 quantisation (kf_ops.h): one thread per (row, 32-element block)
// ---------------------------------------------------------------------------
__global__ void k_quant_mxfp8(const h16 *src, long long ld_src, int rows, int cols, int cols_pad,
                              int transpose, uint8_t *q, long long ldq, uint8_t *scales,
                              long long lds) {
    const int nblk = cols_pad / 32;
    const long long total = (long long)rows * nblk;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        // transposed source (weights): consecutive threads take consecutive rows r, so each
        // of the 32 loads of a block is one coalesced source row; else consecutive blocks
        int r, b;
        if (transpose) {
            b = (int)(i / rows);
            r = (int)(i - (long long)b * rows);
        } else {
            r = (int)(i / nblk);
            b = (int)(i - (long long)r * nblk);
        }
        float v[32];
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int c = 32 * b + j;
            float x = 0.f;
            if (c < cols) x = h2f(transpose ? src[(long long)c * ld_src + r] : src[(long long)r * ld_src + c]);
            v[j] = x;
            amax = fmaxf(amax, fabsf(x));
        }
        const int ex = mx_exponent(amax);
        const float inv = __uint_as_float((unsigned)(127 - ex) << 23);
#pragma unroll
        for (int j = 0; j < 32; ++j) v[j] *= inv;
        uint8_t *qr = q + (long long)r * ldq + 32 * b;
#pragma unroll
        for (int w = 0; w < 4; ++w) *reinterpret_cast<uint2 *>(qr + 8 * w) = pack_e4m3x8(v + 8 * w);
        scales[(long long)r * lds + b] = (uint8_t)(ex + 127);
    }
}

// Row quantisation on 16-byte vectors (source rows 16-byte aligned, cols % 8 == 0): four
// lanes per 32-element block, eight elements each, the block's amax by two lane swaps as in
// the GEMM epilogue's copy, so a wave reads 1 KB of contiguous row bytes per load.
__global__ __launch_bounds__(256) void k_quant_mxfp8_rows_v8(const h16 *src, long long ld_src, int rows, int cols,
                                                             int nblk, uint8_t *q, long long ldq, uint8_t *scales,
                                                             long long lds) {
    const long long total = (long long)rows * nblk * 4;
    const long long S = (long long)gridDim.x * blockDim.x;
    // total is a multiple of 4 and S of 64, so a block's four lanes are live together
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += S) {
        const long long rb = i >> 2;
        const int r = (int)(rb / nblk), b = (int)(rb - (long long)r * nblk), c0 = 32 * b + 8 * (int)(i & 3);
        float v[8];
        if (c0 < cols) {
            const half8 x = *reinterpret_cast<const half8 *>(src + (long long)r * ld_src + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
        }
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
        amax = fmaxf(amax, __shfl_xor(amax, 1));
        amax = fmaxf(amax, __shfl_xor(amax, 2));
        const int ex = mx_exponent(amax);
        const float inv = __uint_as_float((unsigned)(127 - ex) << 23);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= inv;
        *reinterpret_cast<uint2 *>(q + (long long)r * ldq + c0) = pack_e4m3x8(v);
        if ((i & 3) == 0) scales[(long long)r * lds + b] = (uint8_t)(ex + 127);
    }
}

// Weight quantisation of many matrices in one launch (kf_quant_mxfp8_batch): job j owns
// threads [t0[j], t0[j+1]) of the grid, one per (row, 32-element block), rows fastest.
struct QuantJobs {
    KfQuantJob job[KF_QUANT_MAX];
    long long t0[KF_QUANT_MAX + 1];
    int n;
};
__global__ __launch_bounds__(256) void k_quant_mxfp8_batch(QuantJobs J) {
    const long long S = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < J.t0[J.n]; i += S) {
        int j = 0;
        while (j + 1 < J.n && i >= J.t0[j + 1]) ++j;
        const KfQuantJob &Q = J.job[j];
        const long long l = i - J.t0[j];
        const h16 *src = (const h16 *)Q.src;
        int r, b;
        if (Q.transpose) {
            b = (int)(l / Q.rows);
            r = (int)(l - (long long)b * Q.rows);
        } else {
            const int nblk = (Q.cols + 127) / 128 * 4;
            r = (int)(l / nblk);
            b = (int)(l - (long long)r * nblk);
        }
        float v[32];
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 32; ++e) {
            const int c = 32 * b + e;
            float x = 0.f;
            if (c < Q.cols) x = h2f(Q.transpose ? src[(long long)c * Q.ld_src + r] : src[(long long)r * Q.ld_src + c]);
            v[e] = x;
            amax = fmaxf(amax, fabsf(x));
        }
        const int ex = mx_exponent(amax);
        const float inv = __uint_as_float((unsigned)(127 - ex) << 23);
#pragma unroll
        for (int e = 0; e < 32; ++e) v[e] *= inv;
        uint8_t *qr = (uint8_t *)Q.q + (long long)r * Q.ldq + 32 * b;
#pragma unroll
        for (int w = 0; w < 4; ++w) *reinterpret_cast<uint2 *>(qr + 8 * w) = pack_e4m3x8(v + 8 * w);
        Q.scales[(long long)r * Q.lds + b] = (uint8_t)(ex + 127);
    }
}

// Row jobs on 16-byte vectors (cols % 8 == 0, ld_src % 8 == 0, aligned source: host-checked),
// as k_quant_mxfp8_rows_v8: four lanes per 32-element block; J.t0 counts lanes
__global__ __launch_bounds__(256) void k_quant_mxfp8_vbatch(QuantJobs J) {
    const long long S = (long long)gridDim.x * blockDim.x;
    // every job's lane count is a multiple of 4 and S of 64: a block's four lanes are live together
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < J.t0[J.n]; i += S) {
        int j = 0;
        while (j + 1 < J.n && i >= J.t0[j + 1]) ++j;
        const KfQuantJob &Q = J.job[j];
        const long long l = i - J.t0[j], rb = l >> 2;
        const int nblk = (Q.cols + 127) / 128 * 4;
        const int r = (int)(rb / nblk), b = (int)(rb - (long long)r * nblk), c0 = 32 * b + 8 * (int)(l & 3);
        float v[8];
        if (c0 < Q.cols) {
            const half8 x = load_h8((const h16 *)Q.src + (long long)r * Q.ld_src + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
        }
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
        amax = fmaxf(amax, __shfl_xor(amax, 1));
        amax = fmaxf(amax, __shfl_xor(amax, 2));
        const int ex = mx_exponent(amax);
        const float inv = __uint_as_float((unsigned)(127 - ex) << 23);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= inv;
        *reinterpret_cast<uint2 *>((uint8_t *)Q.q + (long long)r * Q.ldq + c0) = pack_e4m3x8(v);
        if ((l & 3) == 0) Q.scales[(long long)r * Q.lds + b] = (uint8_t)(ex + 127);
    }
}

// Transposed jobs (weights W[K][N] -> W8[N][K]) through LDS: a workgroup owns 64 output rows
// r (source columns) x 256 k (8 blocks): the source tile is read as 256 row segments of 128
// bytes, and each output row's 256 bytes are written by 32 consecutive lanes (4 per block,
// the block amax by two lane swaps), so both sides are coalesced.
struct QuantTJobs {
    KfQuantJob job[KF_QUANT_MAX];
    int wg0[KF_QUANT_MAX + 1];  // first workgroup of each job
    int rt[KF_QUANT_MAX];       // 64-row tiles of each job
    int n;
};
__global__ __launch_bounds__(256) void k_quant_mxfp8_tbatch(QuantTJobs J) {
    __shared__ float tile[256][65];
    int j = 0;
    while (j + 1 < J.n && (int)blockIdx.x >= J.wg0[j + 1]) ++j;
    const KfQuantJob &Q = J.job[j];
    const int w = blockIdx.x - J.wg0[j];
    const int r0 = (w % J.rt[j]) * 64, k0 = (w / J.rt[j]) * 256;
    const h16 *src = (const h16 *)Q.src;
    // 2048 16-byte source vectors (8 per 64-row tile row), all loads issued before the LDS
    // writes (rows % 8 == 0, ld_src % 8 == 0, 16-byte aligned source: host-checked)
    half8 xs[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = threadIdx.x + 256 * u, k = k0 + (i >> 3), r = r0 + 8 * (i & 7);
        xs[u] = (k < Q.cols && r < Q.rows) ? load_h8(src + (long long)k * Q.ld_src + r) : half8{};
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = threadIdx.x + 256 * u, kk = i >> 3, rr = 8 * (i & 7);
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[kk][rr + e] = (float)xs[u][e];
    }
    __syncthreads();
    const int kpad = (Q.cols + 127) / 128 * 128;
    for (int i = threadIdx.x; i < 64 * 32; i += 256) {  // i = output row * 32 + block * 4 + quarter
        const int rr = i >> 5, b = (i >> 2) & 7, qq = i & 3, r = r0 + rr, c0 = 32 * b + 8 * qq;
        float v[8];
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] = tile[c0 + e][rr];
            amax = fmaxf(amax, fabsf(v[e]));
        }
        amax = fmaxf(amax, __shfl_xor(amax, 1));
        amax = fmaxf(amax, __shfl_xor(amax, 2));
        const int ex = mx_exponent(amax);
        const float inv = __uint_as_float((unsigned)(127 - ex) << 23);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= inv;
        if (r < Q.rows && k0 + c0 < kpad) {
            *reinterpret_cast<uint2 *>((uint8_t *)Q.q + (long long)r * Q.ldq + k0 + c0) = pack_e4m3x8(v);
            if (qq == 0) Q.scales[(long long)r * Q.lds + (k0 >> 5) + b] = (uint8_t)(ex + 127);
        }
    }
}

static bool quant_args_ok(const void *src, int rows, int cols, const void *q, long long ldq, const uint8_t *scales,
                          long long lds) {
    const int cols_pad = (cols + 127) / 128 * 128;
    return src && q && scales && ldq >= cols_pad && ldq % 16 == 0 && lds >= cols_pad / 32 && !((uintptr_t)q & 7);
}

extern "C" int kf_quant_mxfp8_batch(int n, const KfQuantJob *jobs) {
    kf_take_pending(__func__);
    if (n < 0 || n > KF_QUANT_MAX || (n && !jobs)) {
        kf_report_error("kf_quant_mxfp8_batch: %d jobs (at most %d)", n, KF_QUANT_MAX);
        return -1;
    }
    QuantJobs J{}, VJ{};
    QuantTJobs TJ{};
    long long tot = 0, vtot = 0;
    int twg = 0;
    for (int j = 0; j < n; ++j) {
        const KfQuantJob &Q = jobs[j];
        if (Q.rows < 0 || Q.cols < 0 || ((Q.rows && Q.cols) && !quant_args_ok(Q.src, Q.rows, Q.cols, Q.q, Q.ldq,
                                                                                Q.scales, Q.lds))) {
            kf_report_error("kf_quant_mxfp8_batch: bad job %d (rows=%d cols=%d ldq=%lld lds=%lld)", j, Q.rows, Q.cols,
                            Q.ldq, Q.lds);
            return -1;
        }
        if (!Q.rows || !Q.cols) continue;
        if (Q.transpose && Q.rows % 8 == 0 && Q.ld_src % 8 == 0 && !((uintptr_t)Q.src & 15)) {
            // LDS-tiled: 64 rows x 256 k per workgroup
            TJ.job[TJ.n] = Q;
            TJ.wg0[TJ.n] = twg;
            TJ.rt[TJ.n] = (Q.rows + 63) / 64;
            twg += TJ.rt[TJ.n] * ((Q.cols + 127) / 128 * 128 + 255) / 256;
            ++TJ.n;
        } else if (!Q.transpose && Q.cols % 8 == 0 && Q.ld_src % 8 == 0 && !((uintptr_t)Q.src & 15)) {
            VJ.job[VJ.n] = Q;  // row jobs on 16-byte vectors
            VJ.t0[VJ.n] = vtot;
            vtot += (long long)Q.rows * ((Q.cols + 127) / 128 * 4) * 4;
            ++VJ.n;
        } else {
            J.job[J.n] = Q;
            J.t0[J.n] = tot;
            tot += (long long)Q.rows * ((Q.cols + 127) / 128 * 4);
            ++J.n;
        }
    }
    J.t0[J.n] = tot;
    VJ.t0[VJ.n] = vtot;
    TJ.wg0[TJ.n] = twg;
    if (tot > 0) k_quant_mxfp8_batch<<<kf_blocks(tot, 256, 16384), 256, 0, kf_stream()>>>(J);
    if (vtot > 0) k_quant_mxfp8_vbatch<<<kf_blocks(vtot, 256, 16384), 256, 0, kf_stream()>>>(VJ);
    if (twg > 0) k_quant_mxfp8_tbatch<<<twg, 256, 0, kf_stream()>>>(TJ);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kf_report_error("kf_quant_mxfp8_batch: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}

extern "C" int kf_quant_mxfp8(const void *src, long long ld_src, int rows, int cols, int transpose,
                              void *q, long long ldq, uint8_t *scales, long long lds) {
    kf_take_pending(__func__);
    if (rows <= 0 || cols <= 0) return 0;
    const int cols_pad = (cols + 127) / 128 * 128;
    if (!quant_args_ok(src, rows, cols, q, ldq, scales, lds)) {
        kf_report_error("kf_quant_mxfp8: bad arguments (rows=%d cols=%d ldq=%lld lds=%lld)", rows,
                        cols, ldq, lds);
        return -1;
    }
    const long long total = (long long)rows * (cols_pad / 32);
    if (!transpose && cols % 8 == 0 && ld_src % 8 == 0 && !((uintptr_t)src & 15))
        k_quant_mxfp8_rows_v8<<<kf_blocks(4 * total, 256, 16384), 256, 0, kf_stream()>>>(
            (const h16 *)src, ld_src, rows, cols, cols_pad / 32, (uint8_t *)q, ldq, scales, lds);
    else
        k_quant_mxfp8<<<kf_blocks(total, 256, 16384), 256, 0, kf_stream()>>>(
            (const h16 *)src, ld_src, rows, cols, cols_pad, transpose, (uint8_t *)q, ldq, scales, lds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kf_report_error("kf_quant_mxfp8: %s", hipGetErrorString(e));
        return -1;
    }
    return 0;
}
