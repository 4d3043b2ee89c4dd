// orthonormal.hip — the semi-orthogonal constraint over the flat parameter set
// (include/kf_ops.h kf_orthonormal_constrain): Kaldi's ConstrainOrthonormal for
// every constrained matrix W [K x n] (columns constrained) in one call.
//
// Three launches on the current stream, no host round trip, no atomics:
//   k_ortho_gram    P = W^T W from the fp32 weights on the exact f32-input MFMA (32x32x2): a
//                   workgroup owns 32 rows of P over one chunk of KF_ORTHO_KCHUNK rows of W and
//                   writes its partial tiles to scratch
//   k_ortho_scales  one workgroup per matrix: the chunks' partials summed in chunk order, the
//                   traces in double, s / ratio / nu, Q = P - s^2 I into scratch, err, the
//                   factor 4 nu / s^2 and the stats
//   k_ortho_apply   a workgroup owns 32 rows of W: w32 <- w32 - factor * (W Q) on the same
//                   MFMA, Q read in 32-column tiles from scratch; w16 <- rne(w32)
// A workgroup finds its matrix by a scan of the table (a few dozen entries) in the order the
// host sized the launch by.
//
// Every sum runs in a fixed order (the MFMA's k-ordered fma chain, the chunks in chunk order,
// the traces per thread in element order, the wave by shuffles, the waves through LDS in wave
// order), so two runs on the same inputs give the same bits.
#include "kf_common.h"
#include "../../include/kf_ops.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;        // gram, apply: 4 waves, each a 32 x 32 tile at a time
constexpr int kScaleThreads = 1024;  // k_ortho_scales
constexpr int kKC = KF_ORTHO_KCHUNK;
static_assert(kKC % 32 == 0, "a chunk is whole unrolled rounds of k steps");
typedef float f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ inline int ortho_chunks(int K) { return (K + kKC - 1) / kKC; }
// scratch of one constrained matrix, in floats: the chunks' partial P tiles, then Q
__host__ __device__ inline long long ortho_tile_floats(int K, int n) {
    return (long long)(ortho_chunks(K) + 1) * n * n;
}
__host__ __device__ inline int ortho_gram_wgs(int K, int n) { return ortho_chunks(K) * (n / 32); }
__host__ __device__ inline int ortho_apply_wgs(int K) { return K / 32; }
inline bool ortho_shape_ok(int K, int n) { return K > 0 && n >= 32 && K % 32 == 0 && n % 32 == 0 && n <= K && n <= 512; }
inline size_t ortho_align(size_t b) { return (b + 255) / 256 * 256; }

struct OrthoLoc {
    int m, local;    // matrix, and the workgroup's index within it
    long long soff;  // the matrix's tiles, floats into the tile region of scratch
};
// workgroup b of the gram (apply = false) or the apply launch; false when b is past the table
__device__ __forceinline__ bool ortho_locate(const KfOrthoMat *mats, int nmat, int b, bool apply, OrthoLoc &loc) {
    long long soff = 0;
    for (int m = 0; m < nmat; ++m) {
        const KfOrthoMat t = mats[m];
        if (t.c == 0.f) continue;
        const int cnt = apply ? ortho_apply_wgs(t.K) : ortho_gram_wgs(t.K, t.n);
        if (b < cnt) {
            loc.m = m;
            loc.local = b;
            loc.soff = soff;
            return true;
        }
        b -= cnt;
        soff += ortho_tile_floats(t.K, t.n);
    }
    return false;
}

// 32x32x2 f32 MFMA: lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31];
// register g of lane l holds D[row (g & 3) + 8 (g >> 2) + 4 (l >> 5)][col l & 31]
__device__ __forceinline__ int ortho_drow(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

__global__ __launch_bounds__(kThreads) void k_ortho_gram(const float *__restrict__ w32,
                                                         const KfOrthoMat *__restrict__ mats, int nmat,
                                                         float *__restrict__ tiles) {
    OrthoLoc loc;
    if (!ortho_locate(mats, nmat, blockIdx.x, false, loc)) return;  // the same in every thread
    const KfOrthoMat t = mats[loc.m];
    const int n = t.n, nt = n / 32, ch = loc.local / nt, ti = loc.local % nt;
    const int k0 = ch * kKC, k1 = k0 + kKC < t.K ? k0 + kKC : t.K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const float *W = w32 + t.offset;
    float *part = tiles + loc.soff + (long long)ch * n * n;
    for (int tj = wave; tj < nt; tj += kThreads / 64) {
        // P[ti*32 + i][tj*32 + j] = sum_k W[k][ti*32 + i] W[k][tj*32 + j]: both operands are
        // rows of W read as they lie (32 consecutive floats per half wave)
        const float *pa = W + (long long)(k0 + h) * n + ti * 32 + r;
        const float *pb = W + (long long)(k0 + h) * n + tj * 32 + r;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = k0; k < k1; k += 16) {  // K % 32 == 0: whole rounds of 8 k steps, loads first
            float a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                a[u] = pa[(long long)2 * u * n];
                b[u] = pb[(long long)2 * u * n];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
            pa += 16 * n;
            pb += 16 * n;
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) part[(long long)(ti * 32 + ortho_drow(g, h)) * n + tj * 32 + r] = acc[g];
    }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}
// the workgroup's sum in thread 0: the wave by shuffles, the waves through LDS in wave order
__device__ __forceinline__ double block_sum(double x, double *sh) {
    x = wave_sum(x);
    __syncthreads();  // sh may still be read from the sum before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kScaleThreads / 64; ++w) s += sh[w];
    return s;
}

// Workgroup m takes matrix m. Each thread owns the elements tid, tid + 1024, ... of P: it sums
// the chunks' partials in chunk order, leaves P where Q goes, and after s is known turns its
// own elements into Q, so no thread reads what another wrote.
__global__ __launch_bounds__(kScaleThreads) void k_ortho_scales(const KfOrthoMat *__restrict__ mats, int nmat,
                                                                float *__restrict__ tiles, float *__restrict__ factor,
                                                                float *__restrict__ stats) {
    const int m = blockIdx.x, tid = threadIdx.x;
    const KfOrthoMat t = mats[m];
    __shared__ double sh[kScaleThreads / 64];
    __shared__ double sh_s2;
    if (tid == 0) {  // off, or left untouched: overwritten below otherwise
        factor[m] = 0.f;
        stats[4 * m] = stats[4 * m + 1] = stats[4 * m + 2] = stats[4 * m + 3] = 0.f;
        sh_s2 = -1.0;
    }
    if (t.c == 0.f) return;
    long long soff = 0;
    for (int q = 0; q < m; ++q)
        if (mats[q].c != 0.f) soff += ortho_tile_floats(mats[q].K, mats[q].n);
    const int n = t.n, nn = n * n, nch = ortho_chunks(t.K);
    const float *part = tiles + soff;
    float *Q = tiles + soff + (long long)nch * nn;
    double tp = 0.0, tpp = 0.0;
    for (int e = tid; e < nn; e += kScaleThreads) {
        float p = part[e];
        for (int c = 1; c < nch; ++c) p += part[(long long)c * nn + e];
        Q[e] = p;
        if (e / n == e % n) tp += (double)p;
        tpp += (double)p * (double)p;
    }
    tp = block_sum(tp, sh);
    tpp = block_sum(tpp, sh);
    if (tid == 0) {
        double s = 0.0, ratio = 1.0, nu = 0.125;
        if (t.c < 0.f) {
            s = sqrt(tpp / tp);
            ratio = tpp * (double)n / (tp * tp);
            if (ratio > 1.02) nu *= 0.5;
            if (ratio > 1.1) nu *= 0.5;
        } else {
            s = (double)t.c;
        }
        // an all-zero matrix (tP == 0) or a non-finite scale: left untouched, s = 0
        if (tp != 0.0 && isfinite(s) && s > 0.0 && isfinite(4.0 * nu / (s * s))) {
            factor[m] = (float)(4.0 * nu / (s * s));
            stats[4 * m] = (float)s;
            stats[4 * m + 1] = (float)ratio;
            stats[4 * m + 3] = (float)nu;
            sh_s2 = s * s;
        }
    }
    __syncthreads();
    const double s2 = sh_s2;
    if (s2 < 0.0) return;  // the same in every thread
    double e2 = 0.0;
    for (int e = tid; e < nn; e += kScaleThreads) {
        double q = (double)Q[e];
        if (e / n == e % n) q -= s2;
        const float qf = (float)q;
        Q[e] = qf;
        e2 += (double)qf * (double)qf;
    }
    e2 = block_sum(e2, sh);
    if (tid == 0) stats[4 * m + 2] = (float)sqrt(e2);
}

// w16 = rne(the stored fp32 w): the barrier keeps hipcc from folding the update into
// v_fma_mixlo_f16, which rounds the exact w - f*x to fp16 once and differs from rne(w32) at
// near-ties (as in k_sgd_flat and k_upd_apply)
__device__ __forceinline__ float ortho_weight(float w, float f, float x) {
    float r = w - f * x;
    asm volatile("" : "+v"(r));
    return r;
}

// column k of row r of the workgroup's row block in LDS: rows are rotated by their index, so
// the 32 rows of one k lie in 32 banks (n % 32 == 0) without padding the 64 KiB block of n = 512
__device__ __forceinline__ int ortho_lds(int r, int k, int n) {
    int kk = k + r;
    if (kk >= n) kk -= n;
    return r * n + kk;
}

// The update is in place, and row i of W - f W Q depends on row i of W alone: the workgroup
// reads its 32 rows completely into LDS before it writes any of them, and no other workgroup
// touches these rows. Q (n x n, up to 1 MiB: not held in LDS whole) is read from scratch one
// 32-column tile per wave.
__global__ __launch_bounds__(kThreads) void k_ortho_apply(float *__restrict__ w32, h16 *__restrict__ w16,
                                                          const KfOrthoMat *__restrict__ mats, int nmat,
                                                          const float *__restrict__ tiles,
                                                          const float *__restrict__ factor) {
    extern __shared__ float sw[];  // [32][n], ortho_lds
    OrthoLoc loc;
    if (!ortho_locate(mats, nmat, blockIdx.x, true, loc)) return;  // the same in every thread
    const float f = factor[loc.m];
    if (f == 0.f) return;  // left untouched (k_ortho_scales)
    const KfOrthoMat t = mats[loc.m];
    const int n = t.n, nt = n / 32;
    const long long base = t.offset + (long long)loc.local * 32 * n;  // the row block's first element
    const float *Q = tiles + loc.soff + (long long)ortho_chunks(t.K) * n * n;
    for (int idx = threadIdx.x; idx < 32 * n; idx += kThreads) {
        const int rr = idx / n, k = idx - rr * n;
        sw[ortho_lds(rr, k, n)] = w32[base + idx];
    }
    __syncthreads();  // the whole row block is read; nothing of it is written before this point
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    for (int tj = wave; tj < nt; tj += kThreads / 64) {
        // X[i][tj*32 + j] = sum_k W[i][k] Q[k][tj*32 + j]
        const float *pb = Q + (long long)h * n + tj * 32 + r;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < n; k += 16) {  // n % 32 == 0: whole rounds of 8 k steps, loads first
            float a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                a[u] = sw[ortho_lds(r, k + 2 * u + h, n)];
                b[u] = pb[(long long)2 * u * n];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
            pb += 16 * n;
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = ortho_drow(g, h), col = tj * 32 + r;
            const float w = ortho_weight(sw[ortho_lds(row, col, n)], f, acc[g]);
            w32[base + (long long)row * n + col] = w;
            w16[base + (long long)row * n + col] = f2h(w);
        }
    }
}

// the table's launch sizes; false (with the error text set) when an entry is not supported
bool ortho_plan(const KfOrthoMat *mats, int nmat, long long n_params, long long &gram, long long &apply,
                long long &tile_floats, int &max_n, const char *who) {
    gram = apply = tile_floats = 0;
    max_n = 0;
    for (int m = 0; m < nmat; ++m) {
        const KfOrthoMat &t = mats[m];
        if (t.c == 0.f) continue;
        if (!isfinite(t.c)) {
            kf_report_error("%s: matrix %d has a non-finite constraint value", who, m);
            return false;
        }
        if (!ortho_shape_ok(t.K, t.n)) {
            kf_report_error("%s: matrix %d is %d x %d; a constrained matrix needs K %% 32 == 0, n %% 32 == 0, "
                            "32 <= n <= K and n <= 512 (n > K: transposed case not supported)", who, m, t.K, t.n);
            return false;
        }
        if (t.offset < 0 || (n_params >= 0 && t.offset + (long long)t.K * t.n > n_params)) {
            kf_report_error("%s: matrix %d (offset %lld, %d x %d) lies outside the %lld parameters", who, m, t.offset,
                            t.K, t.n, n_params);
            return false;
        }
        gram += ortho_gram_wgs(t.K, t.n);
        apply += ortho_apply_wgs(t.K);
        tile_floats += ortho_tile_floats(t.K, t.n);
        if (t.n > max_n) max_n = t.n;
    }
    return true;
}

}  // namespace

extern "C" long long kf_orthonormal_scratch_bytes(const KfOrthoMat *mats, int nmat) {
    long long gram, apply, tf;
    int max_n;
    if (nmat < 0 || (nmat > 0 && !mats)) return -1;
    if (!ortho_plan(mats, nmat, -1, gram, apply, tf, max_n, "kf_orthonormal_scratch_bytes")) return -1;
    return (long long)ortho_align((size_t)nmat * 4) + tf * 4;
}

extern "C" int kf_orthonormal_constrain(float *w32, void *w16, long long n_params, const KfOrthoMat *mats,
                                        const KfOrthoMat *mats_dev, int nmat, void *scratch, float *stats) {
    kf_take_pending(__func__);
    if (n_params < 0 || nmat < 0 || (nmat > 0 && (!mats || !mats_dev))) {
        kf_report_error("kf_orthonormal_constrain: bad arguments (%lld parameters, %d matrices)", n_params, nmat);
        return -1;
    }
    long long gram, apply, tf;
    int max_n;
    if (!ortho_plan(mats, nmat, n_params, gram, apply, tf, max_n, "kf_orthonormal_constrain")) return -1;
    if (gram == 0) return 0;  // nothing is constrained: no launch
    if (!w32 || !w16 || !scratch || !stats || gram > 0x7fffffffll || apply > 0x7fffffffll || (uintptr_t)scratch % 16 ||
        (uintptr_t)w32 % 4 || (uintptr_t)w16 % 2) {
        kf_report_error("kf_orthonormal_constrain: null or misaligned buffer (scratch 16 bytes), or more than 2^31 "
                        "workgroups");
        return -1;
    }
    float *factor = (float *)scratch;
    float *tiles = (float *)((char *)scratch + ortho_align((size_t)nmat * 4));
    k_ortho_gram<<<(unsigned)gram, kThreads, 0, kf_stream()>>>(w32, mats_dev, nmat, tiles);
    k_ortho_scales<<<(unsigned)nmat, kScaleThreads, 0, kf_stream()>>>(mats_dev, nmat, tiles, factor, stats);
    k_ortho_apply<<<(unsigned)apply, kThreads, (size_t)32 * max_n * 4, kf_stream()>>>(w32, (h16 *)w16, mats_dev, nmat,
                                                                                      tiles, factor);
    return hipGetLastError() == hipSuccess ? 0 : (kf_report_error("kf_orthonormal_constrain: launch failed"), -1);
}
