// natgrad_conv.hip — natural gradient on the parameter side (include/kf_ops.h kf_ng_conv_*; DESIGN.md
// §32): Kaldi's TimeHeightConvolutionComponent preconditions the finished parameter derivative
// G = [dW ; db] [Din x N] itself, first with the rows of G^T as the data (in side), then with the
// rows of the unscaled G1 = G - W_in^T W_in G (out side). Batched over a table of components; the
// matrices are small (at most [2305 x 256] with ranks up to 96) and few, so every stage splits one
// component over workgroups and leaves partials that the next stage sums in a fixed order:
//
//   1 k_ngc_in_part   P[chunk] = W_in G per 256 rows of G and |G|^2 per chunk, in double
//   2 k_ngc_in_sum    P = sum of the chunks (chunk order), kept in double and in fp32
//   3 k_ngc_g1q       per 32 rows of G: G1 = G - W_in^T P in double, rounded once to fp32 (scratch and
//                     LDS), |G1|^2 of the block, Q = G1 W_out^T in double from the LDS tile and W_out
//                     staged through LDS 32 columns at a time; beside them the tiles of L_in = P P^T
//                     and the head of the in side's statistics
//   4 k_ngc_out_part  L_out = Q^T Q per 256 rows in double; on updating steps JT_out = G1^T Q per 256
//                     rows and JT_in = G P^T on the exact f32-input MFMA, a 32 x 32 tile per wave
//   5 k_ngc_out_sum   L_out, |G1|^2 and JT_out: the partials in order, in double, rounded once
//   (kf_ng_scales)
//   6 k_ngc_final     G^ = gamma_in gamma_out (G1 - Q W_out) in double, into g
//
// g is read-only until stage 6. Every sum runs in a fixed order, so two runs give the same bits.
#include "natgrad_dev.h"

namespace {

constexpr int kG1Cols = 256;  // columns of G a workgroup of stage 3 holds in LDS at a time
constexpr int kWtCols = 32;   // columns of W_out staged at a time
constexpr int kStages = 6;

// where one component's intermediates lie in scratch (byte offsets, multiples of 16)
struct NgcLay {
    long long ppart, trxin, pd, p32, g1, qd, q32, trxout, lpart, jtpart, bytes;
};
struct NgcDims {
    int Din, N, Np, Dp, nch, ngr, nrb, Rpi, Rpo;  // Rp of a side that is left alone: 0
};
__host__ __device__ inline NgcDims ngc_dims(const KfNgComp &c, const KfNgPre *pres) {
    NgcDims d;
    d.Din = ng_din(c);
    d.N = c.N;
    d.Np = ng_up32(c.N);
    d.Dp = ng_up32(d.Din);
    d.nch = ng_pchunks(d.Din);
    d.ngr = ng_colgroups(c.N);
    d.nrb = d.Dp / 32;
    d.Rpi = c.pre_in >= 0 ? ng_rp(pres[c.pre_in].R) : 0;
    d.Rpo = c.pre_out >= 0 ? ng_rp(pres[c.pre_out].R) : 0;
    return d;
}
__host__ __device__ inline long long ngc_up16(long long b) { return (b + 15) / 16 * 16; }
__host__ __device__ inline NgcLay ngc_lay(const NgcDims &d) {
    NgcLay l;
    long long at = 0;
    auto take = [&](long long bytes) {
        const long long was = at;
        at += ngc_up16(bytes);
        return was;
    };
    l.ppart = take(8ll * d.nch * d.Rpi * d.Np);
    l.trxin = take(8ll * d.nch * d.ngr);
    l.pd = take(8ll * d.Rpi * d.Np);
    l.p32 = take(4ll * d.Rpi * d.Np);
    l.g1 = take(4ll * d.Dp * d.N);
    l.qd = take(8ll * d.Dp * d.Rpo);
    l.q32 = take(4ll * d.Dp * d.Rpo);
    l.trxout = take(8ll * d.nrb);
    l.lpart = take(8ll * d.nch * d.Rpo * d.Rpo);
    l.jtpart = take(4ll * d.nch * d.Np * d.Rpo);
    l.bytes = at;
    return l;
}
// workgroups of one component in a stage
__host__ __device__ inline long long ngc_wgs(const NgcDims &d, int stage, int update) {
    const long long ti = d.Rpi / 32, to = d.Rpo / 32;
    switch (stage) {
    case 1: return (long long)d.ngr * d.nch * ti;
    case 2: return d.Rpi ? d.Np / 32 : 0;
    case 3: return d.nrb + ti * ti;
    case 4: return d.nch * to * to + (update && d.Rpo ? (long long)d.nch * (d.Np / 32) : 0) + (update && d.Rpi ? d.nrb : 0);
    case 5: return d.Rpo ? 1 + (update ? d.Np / 32 : 0) : 0;
    default: return (long long)d.nrb * d.ngr;
    }
}

// this workgroup's component, its index within the component's workgroups and its scratch
struct NgcAt {
    KfNgComp c;
    NgcDims d;
    NgcLay l;
    long long b;
    char *s;
    bool ok;
};
__device__ __forceinline__ NgcAt ngc_find(const KfNgComp *comps, int ncomp, const KfNgPre *pres, int stage, int update,
                                          void *scratch) {
    NgcAt a;
    a.b = blockIdx.x;
    a.s = (char *)scratch;
    a.ok = false;
    for (int m = 0; m < ncomp; ++m) {
        a.c = comps[m];
        a.d = ngc_dims(a.c, pres);
        a.l = ngc_lay(a.d);
        const long long cnt = ngc_wgs(a.d, stage, update);
        if (a.b < cnt) {
            a.ok = true;
            break;
        }
        a.b -= cnt;
        a.s += a.l.bytes;
    }
    return a;
}

// out[2a + b] = sum_{i0 <= i < i1} A(r0 + tr + 16 a, i) A(s0 + ts + 16 b, i) in index order: a 32 x 32
// tile of a Gram matrix per workgroup, 2 x 2 per thread. (r, s) and (s, r) are the same expression.
template <class FA>
__device__ __forceinline__ void ngc_gram(int i0, int i1, int r0, int s0, FA A, double out[4]) {
    const int tr = threadIdx.x >> 4, ts = threadIdx.x & 15;
    out[0] = out[1] = out[2] = out[3] = 0.0;
    for (int i = i0; i < i1; ++i) {
        const double a0 = A(r0 + tr, i), a1 = A(r0 + tr + 16, i), b0 = A(s0 + ts, i), b1 = A(s0 + ts + 16, i);
        out[0] += a0 * b0;
        out[1] += a0 * b1;
        out[2] += a1 * b0;
        out[3] += a1 * b1;
    }
}
template <class T>
__device__ __forceinline__ void ngc_gram_store(const double out[4], int r0, int s0, T *dst, int ld) {
    const int tr = threadIdx.x >> 4, ts = threadIdx.x & 15;
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[(long long)(r0 + tr + 16 * (q >> 1)) * ld + s0 + ts + 16 * (q & 1)] = (T)out[q];
}

// the head of a side's statistics: trX, the rows of X and this preconditioner's history in samples
__device__ __forceinline__ void ngc_head(float *st, double trx, int rows, float nmb) {
    st[0] = (float)trx;
    st[1] = (float)rows;
    st[KF_NG_STAT_HISTORY] = nmb * (float)rows;
}

// ---------------------------------------------------------------- 1: partial P, |G|^2
// As pass 1 of k_ng_apply: a thread owns one column and 16 ranks of the workgroup's 32 ranks x 128
// columns over one chunk of Din. The first rank tile's workgroups also sum the squares they read.
__global__ __launch_bounds__(kThreads) void k_ngc_in_part(const float *__restrict__ g, const KfNgComp *__restrict__ comps,
                                                          int ncomp, const KfNgPre *__restrict__ pres,
                                                          const float *__restrict__ w32, void *scratch) {
    __shared__ double sh[kThreads / 64];
    const NgcAt a = ngc_find(comps, ncomp, pres, 1, 0, scratch);
    if (!a.ok) return;  // the same in every thread
    const NgcDims &d = a.d;
    const KfNgPre pi = pres[a.c.pre_in];
    const int cg = (int)(a.b % d.ngr), ch = (int)((a.b / d.ngr) % d.nch), rt = (int)(a.b / ((long long)d.ngr * d.nch));
    const int n = cg * 128 + (threadIdx.x & 127), rb = rt * 32 + (threadIdx.x >> 7) * 16;
    const int k0 = ch * kPChunk, k1 = k0 + kPChunk < d.Din ? k0 + kPChunk : d.Din;
    const float *W = w32 + pi.w_off + (long long)rb * d.Din;
    double acc[16], sq = 0.0;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0;
    if (n < d.N) {
        for (int k = k0; k < k1; ++k) {
            const double gk = (double)g[ng_gidx(a.c, k, n)];
            if (threadIdx.x < 128) sq += gk * gk;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[rr] += (double)W[(long long)rr * d.Din + k] * gk;
        }
    }
    if (n < d.Np) {
        double *Pc = (double *)(a.s + a.l.ppart) + (long long)ch * d.Rpi * d.Np;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) Pc[(long long)(rb + rr) * d.Np + n] = acc[rr];
    }
    if (rt == 0) {  // the same in every thread
        sq = block_sum_all(sq, sh, kThreads / 64);
        if (threadIdx.x == 0) ((double *)(a.s + a.l.trxin))[ch * d.ngr + cg] = sq;
    }
}

// ---------------------------------------------------------------- 2: P
// 32 columns of P per workgroup: the chunks in chunk order, kept in double (G1, L_in) and rounded
// to fp32 (the MFMA operand of JT_in)
__global__ __launch_bounds__(kThreads) void k_ngc_in_sum(const KfNgComp *__restrict__ comps, int ncomp,
                                                         const KfNgPre *__restrict__ pres, void *scratch) {
    const NgcAt a = ngc_find(comps, ncomp, pres, 2, 0, scratch);
    if (!a.ok) return;
    const NgcDims &d = a.d;
    const int n = (int)a.b * 32 + (threadIdx.x & 31);
    const double *part = (const double *)(a.s + a.l.ppart);
    double *Pd = (double *)(a.s + a.l.pd);
    float *P32 = (float *)(a.s + a.l.p32);
    const long long stride = (long long)d.Rpi * d.Np;
    for (int r = threadIdx.x >> 5; r < d.Rpi; r += kThreads / 32) {
        double s = 0.0;
        for (int q = 0; q < d.nch; ++q) s += part[q * stride + (long long)r * d.Np + n];
        Pd[(long long)r * d.Np + n] = s;
        P32[(long long)r * d.Np + n] = (float)s;
    }
}

// ---------------------------------------------------------------- 3: G1, Q, L_in
__global__ __launch_bounds__(kThreads) void k_ngc_g1q(const float *__restrict__ g, const KfNgComp *__restrict__ comps,
                                                      int ncomp, const KfNgPre *__restrict__ pres,
                                                      const float *__restrict__ w32, float nmb, float *__restrict__ stat,
                                                      void *scratch) {
    __shared__ float g1s[32][kG1Cols + 1];  // the block of G1, fp32 as it is stored
    __shared__ float wt[kWtCols][KF_NG_MAX_RANK + 1];  // W_out^T, 32 columns of it
    __shared__ double sh[kThreads / 64];
    const NgcAt a = ngc_find(comps, ncomp, pres, 3, 0, scratch);
    if (!a.ok) return;
    const NgcDims &d = a.d;
    const int tid = threadIdx.x;
    if (a.b >= d.nrb) {
        // a 32 x 32 tile of L_in = P P^T over all of N; the first tile also sums |G|^2
        const KfNgPre pi = pres[a.c.pre_in];
        const int ti = d.Rpi / 32, tile = (int)(a.b - d.nrb), r0 = tile / ti * 32, s0 = tile % ti * 32;
        const double *Pd = (const double *)(a.s + a.l.pd);
        float *st = stat + pi.st_off;
        double out[4];
        ngc_gram(0, d.N, r0, s0, [&](int r, int i) { return Pd[(long long)r * d.Np + i]; }, out);
        ngc_gram_store(out, r0, s0, st + KF_NG_STAT_L, d.Rpi);
        if (tile == 0 && tid == 0) {
            const double *part = (const double *)(a.s + a.l.trxin);
            double trx = 0.0;
            for (int q = 0; q < d.nch * d.ngr; ++q) trx += part[q];
            ngc_head(st, trx, d.N, nmb);
        }
        return;
    }
    const int i0 = (int)a.b * 32;
    const double *Pd = (const double *)(a.s + a.l.pd);
    float *G1 = (float *)(a.s + a.l.g1);
    const float *Win = d.Rpi ? w32 + pres[a.c.pre_in].w_off : nullptr;
    const float *Wout = d.Rpo ? w32 + pres[a.c.pre_out].w_off : nullptr;
    // Q: a thread owns one rank and 32 / ngrp rows
    const int ngrp = d.Rpo ? kThreads / d.Rpo : 1, rpg = 32 / ngrp;
    const int qr = d.Rpo ? tid % d.Rpo : 0, qg = d.Rpo ? tid / d.Rpo : ngrp;
    double qacc[16], sq = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) qacc[q] = 0.0;
    for (int c0 = 0; c0 < d.N; c0 += kG1Cols) {
        // G1 = G - W_in^T P in double, a thread per column: where gamma is large this is a small
        // difference (k_ng_apply pass 2)
        const int n = c0 + tid;
        double acc[32];
#pragma unroll
        for (int ii = 0; ii < 32; ++ii) acc[ii] = n < d.N && i0 + ii < d.Din ? (double)g[ng_gidx(a.c, i0 + ii, n)] : 0.0;
        if (n < d.N) {
            for (int k = 0; k < d.Rpi; ++k) {
                const double pk = Pd[(long long)k * d.Np + n];
#pragma unroll
                for (int ii = 0; ii < 32; ++ii)
                    if (i0 + ii < d.Din) acc[ii] -= (double)Win[(long long)k * d.Din + i0 + ii] * pk;
            }
        }
        __syncthreads();  // the tile may still be read from the columns before
#pragma unroll
        for (int ii = 0; ii < 32; ++ii) {
            const float v = (float)acc[ii];
            g1s[ii][tid] = v;
            sq += (double)v * (double)v;
            if (n < d.N && i0 + ii < d.Din) G1[(long long)(i0 + ii) * d.N + n] = v;
        }
        // Q += G1[:, c0 ..] W_out[:, c0 ..]^T in double
        for (int n0 = c0; d.Rpo && n0 < d.N && n0 < c0 + kG1Cols; n0 += kWtCols) {
            __syncthreads();  // g1s is written; wt is no longer read
            for (int r = tid >> 5; r < d.Rpo; r += kThreads / 32) {
                const int nn = n0 + (tid & 31);
                wt[tid & 31][r] = nn < d.N ? Wout[(long long)r * d.N + nn] : 0.f;
            }
            __syncthreads();
            if (qg < ngrp) {
                for (int nn = 0; nn < kWtCols; ++nn) {
                    const double w = (double)wt[nn][qr];
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (q < rpg) qacc[q] += (double)g1s[qg * rpg + q][n0 - c0 + nn] * w;
                }
            }
        }
    }
    if (d.Rpo) {
        sq = block_sum_all(sq, sh, kThreads / 64);
        if (tid == 0) ((double *)(a.s + a.l.trxout))[a.b] = sq;
        if (qg < ngrp) {
            double *Qd = (double *)(a.s + a.l.qd);
            float *Q32 = (float *)(a.s + a.l.q32);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (q < rpg) {
                    const long long at = (long long)(i0 + qg * rpg + q) * d.Rpo + qr;
                    Qd[at] = qacc[q];
                    Q32[at] = (float)qacc[q];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- 4: partial L_out, JT
__global__ __launch_bounds__(kThreads) void k_ngc_out_part(const float *__restrict__ g, const KfNgComp *__restrict__ comps,
                                                           int ncomp, const KfNgPre *__restrict__ pres, int update,
                                                           float *__restrict__ stat, void *scratch) {
    const NgcAt a = ngc_find(comps, ncomp, pres, 4, update, scratch);
    if (!a.ok) return;
    const NgcDims &d = a.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int to = d.Rpo / 32;
    long long b = a.b;
    if (b < (long long)d.nch * to * to) {  // a tile of Q^T Q over one chunk of rows
        const int ch = (int)(b / (to * to)), tile = (int)(b % (to * to)), r0 = tile / to * 32, s0 = tile % to * 32;
        const int k0 = ch * kPChunk, k1 = k0 + kPChunk < d.Din ? k0 + kPChunk : d.Din;
        const double *Qd = (const double *)(a.s + a.l.qd);
        double out[4];
        ngc_gram(k0, k1, r0, s0, [&](int rr, int i) { return Qd[(long long)i * d.Rpo + rr]; }, out);
        ngc_gram_store(out, r0, s0, (double *)(a.s + a.l.lpart) + (long long)ch * d.Rpo * d.Rpo, d.Rpo);
        return;
    }
    b -= (long long)d.nch * to * to;
    const long long njo = d.Rpo ? (long long)d.nch * (d.Np / 32) : 0;  // (update != 0: a workgroup past L_out's)
    if (b < njo) {
        // JT_out[32 columns of G1][rank tile wave] over one chunk of rows: a chain of at most 256
        if (wave >= to) return;
        const int ch = (int)(b / (d.Np / 32)), n0 = (int)(b % (d.Np / 32)) * 32;
        const int k0 = ch * kPChunk, k1 = k0 + kPChunk < d.Din ? k0 + kPChunk : d.Din;
        const float *G1 = (const float *)(a.s + a.l.g1) + (long long)k0 * d.N;
        const float *Q = (const float *)(a.s + a.l.q32) + (long long)k0 * d.Rpo + wave * 32;
        const bool col = n0 + r < d.N;
        const f32x16 acc = ng_tile(
            k1 - k0, [&](int i, int k) { return col ? G1[(long long)k * d.N + n0 + i] : 0.f; },
            [&](int k, int j) { return Q[(long long)k * d.Rpo + j]; });
        float *part = (float *)(a.s + a.l.jtpart) + (long long)ch * d.Np * d.Rpo;
#pragma unroll
        for (int q = 0; q < 16; ++q) part[(long long)(n0 + ng_drow(q, h)) * d.Rpo + wave * 32 + r] = acc[q];
        return;
    }
    b -= njo;
    // JT_in[32 rows of G][rank tile wave] = G P^T over all of N
    if (wave >= d.Rpi / 32) return;
    const KfNgPre pi = pres[a.c.pre_in];
    const int i0 = (int)b * 32;
    const float *P = (const float *)(a.s + a.l.p32) + (long long)wave * 32 * d.Np;
    const bool row = i0 + r < d.Din;
    const f32x16 acc = ng_tile(
        d.N, [&](int i, int k) { return row ? g[ng_gidx(a.c, i0 + i, k)] : 0.f; },
        [&](int k, int j) { return P[(long long)j * d.Np + k]; });
    float *JT = stat + pi.st_off + KF_NG_STAT_JT(d.Rpi);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = i0 + ng_drow(q, h);
        if (i < d.Din) JT[(long long)i * d.Rpi + wave * 32 + r] = acc[q];
    }
}

// ---------------------------------------------------------------- 5: L_out, |G1|^2, JT_out
__global__ __launch_bounds__(kThreads) void k_ngc_out_sum(const KfNgComp *__restrict__ comps, int ncomp,
                                                          const KfNgPre *__restrict__ pres, int update, float nmb,
                                                          float *__restrict__ stat, void *scratch) {
    __shared__ double sh[kThreads / 64];
    const NgcAt a = ngc_find(comps, ncomp, pres, 5, update, scratch);
    if (!a.ok) return;
    const NgcDims &d = a.d;
    float *st = stat + pres[a.c.pre_out].st_off;
    const int rr = d.Rpo * d.Rpo;
    if (a.b == 0) {
        const double *part = (const double *)(a.s + a.l.lpart);
        for (int idx = threadIdx.x; idx < rr; idx += kThreads) {
            double s = 0.0;
            for (int q = 0; q < d.nch; ++q) s += part[(long long)q * rr + idx];
            st[KF_NG_STAT_L + idx] = (float)s;
        }
        const double *tp = (const double *)(a.s + a.l.trxout);
        double s = 0.0;
        for (int q = threadIdx.x; q < d.nrb; q += kThreads) s += tp[q];
        s = block_sum_all(s, sh, kThreads / 64);
        if (threadIdx.x == 0) ngc_head(st, s, d.Din, nmb);
        return;
    }
    const int n0 = (int)(a.b - 1) * 32;
    const float *part = (const float *)(a.s + a.l.jtpart);
    float *JT = st + KF_NG_STAT_JT(d.Rpo);
    for (int idx = threadIdx.x; idx < 32 * d.Rpo; idx += kThreads) {
        const int n = n0 + idx / d.Rpo;
        if (n >= d.N) break;
        const long long at = (long long)n * d.Rpo + idx % d.Rpo;
        double s = 0.0;
        for (int q = 0; q < d.nch; ++q) s += (double)part[(long long)q * d.Np * d.Rpo + at];
        JT[at] = (float)s;
    }
}

// ---------------------------------------------------------------- 6: G^
// a thread owns one column and 16 rows of the workgroup's 32 x 128 block, as k_ng_apply pass 2
__global__ __launch_bounds__(kThreads) void k_ngc_final(float *__restrict__ g, const KfNgComp *__restrict__ comps, int ncomp,
                                                        const KfNgPre *__restrict__ pres, const float *__restrict__ w32,
                                                        const float *__restrict__ report, const void *scratch) {
    const NgcAt a = ngc_find(comps, ncomp, pres, 6, 0, (void *)scratch);
    if (!a.ok) return;
    const NgcDims &d = a.d;
    const int n = (int)(a.b % d.ngr) * 128 + (threadIdx.x & 127), ib = (int)(a.b / d.ngr) * 32 + (threadIdx.x >> 7) * 16;
    if (n >= d.N) return;
    const float *G1 = (const float *)(a.s + a.l.g1);
    const double *Qd = (const double *)(a.s + a.l.qd) + (long long)ib * d.Rpo;
    double acc[16];
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) acc[ii] = ib + ii < d.Din ? (double)G1[(long long)(ib + ii) * d.N + n] : 0.0;
    if (d.Rpo) {
        const float *W = w32 + pres[a.c.pre_out].w_off;
        for (int k = 0; k < d.Rpo; ++k) {
            const double wk = (double)W[(long long)k * d.N + n];
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) acc[ii] -= Qd[(long long)ii * d.Rpo + k] * wk;
        }
    }
    double scale = 1.0;
    if (a.c.pre_in >= 0) scale *= (double)report[(long long)KF_NG_REPORT * a.c.pre_in];
    if (a.c.pre_out >= 0) scale *= (double)report[(long long)KF_NG_REPORT * a.c.pre_out];
#pragma unroll
    for (int ii = 0; ii < 16; ++ii)
        if (ib + ii < d.Din) g[ng_gidx(a.c, ib + ii, n)] = (float)(acc[ii] * scale);
}

// ---------------------------------------------------------------- host side
bool ngc_check(const KfNgComp *comps, int ncomp, const KfNgPre *pres, int npre, long long n_grad, int update,
               long long wgs[kStages + 1], long long &bytes, const char *who) {
    bytes = 0;
    for (int q = 0; q <= kStages; ++q) wgs[q] = 0;
    if (ncomp < 0 || (ncomp > 0 && !comps)) {
        kf_report_error("%s: bad component table (%d entries)", who, ncomp);
        return false;
    }
    for (int m = 0; m < ncomp; ++m) {
        const KfNgComp &c = comps[m];
        const bool in_ok = c.pre_in < 0 || (c.pre_in < npre && pres[c.pre_in].D == ng_din(c));
        const bool out_ok = c.pre_out < 0 || (c.pre_out < npre && pres[c.pre_out].D == c.N);
        if (c.K < 1 || c.N < 1 || !in_ok || !out_ok || (c.pre_in < 0 && c.pre_out < 0)) {
            kf_report_error("%s: component %d (%d x %d) does not match its preconditioners", who, m, c.K, c.N);
            return false;
        }
        if (c.dw_off < 0 || (n_grad >= 0 && (c.dw_off + (long long)c.K * c.N > n_grad ||
                                             (c.db_off >= 0 && c.db_off + c.N > n_grad)))) {
            kf_report_error("%s: component %d lies outside the %lld gradient elements", who, m, n_grad);
            return false;
        }
        const NgcDims d = ngc_dims(c, pres);
        for (int q = 1; q <= kStages; ++q) wgs[q] += ngc_wgs(d, q, update);
        bytes += ngc_lay(d).bytes;
    }
    for (int q = 1; q <= kStages; ++q)
        if (wgs[q] > 0x7fffffffll) {
            kf_report_error("%s: more than 2^31 workgroups", who);
            return false;
        }
    return true;
}

}  // namespace

extern "C" long long kf_ng_conv_scratch_bytes(const KfNgComp *comps, int ncomp, const KfNgPre *pres, int npre) {
    long long wgs[kStages + 1], bytes;
    if (!ng_check_pres(pres, npre, __func__) || !ngc_check(comps, ncomp, pres, npre, -1, 1, wgs, bytes, __func__)) return -1;
    return (long long)ng_align((size_t)bytes);
}

extern "C" int kf_ng_conv_stats(const float *g, long long n_grad, const KfNgComp *comps, const KfNgComp *comps_dev,
                                int ncomp, const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const float *w32,
                                float num_minibatches_history, int update, float *stat, void *scratch) {
    kf_take_pending(__func__);
    long long wgs[kStages + 1], bytes;
    if (n_grad < 0 || !(num_minibatches_history > 0.f)) {
        kf_report_error("kf_ng_conv_stats: bad arguments");
        return -1;
    }
    update = update ? 1 : 0;
    if (!ng_check_pres(pres, npre, __func__) || !ngc_check(comps, ncomp, pres, npre, n_grad, update, wgs, bytes, __func__))
        return -1;
    if (ncomp == 0) return 0;
    if (!g || !comps_dev || !pres_dev || !w32 || !stat || !scratch || (uintptr_t)scratch % 16) {
        kf_report_error("kf_ng_conv_stats: null or misaligned buffer (scratch 16 bytes)");
        return -1;
    }
    hipStream_t st = kf_stream();
    if (wgs[1]) {
        k_ngc_in_part<<<(unsigned)wgs[1], kThreads, 0, st>>>(g, comps_dev, ncomp, pres_dev, w32, scratch);
        k_ngc_in_sum<<<(unsigned)wgs[2], kThreads, 0, st>>>(comps_dev, ncomp, pres_dev, scratch);
    }
    k_ngc_g1q<<<(unsigned)wgs[3], kThreads, 0, st>>>(g, comps_dev, ncomp, pres_dev, w32, num_minibatches_history, stat,
                                                     scratch);
    if (wgs[4]) k_ngc_out_part<<<(unsigned)wgs[4], kThreads, 0, st>>>(g, comps_dev, ncomp, pres_dev, update, stat, scratch);
    if (wgs[5])
        k_ngc_out_sum<<<(unsigned)wgs[5], kThreads, 0, st>>>(comps_dev, ncomp, pres_dev, update, num_minibatches_history,
                                                             stat, scratch);
    return ng_launched(__func__);
}

extern "C" int kf_ng_conv_apply(float *g, long long n_grad, const KfNgComp *comps, const KfNgComp *comps_dev, int ncomp,
                                const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const float *w32,
                                const float *report, const void *scratch) {
    kf_take_pending(__func__);
    long long wgs[kStages + 1], bytes;
    if (n_grad < 0) {
        kf_report_error("kf_ng_conv_apply: bad arguments");
        return -1;
    }
    if (!ng_check_pres(pres, npre, __func__) || !ngc_check(comps, ncomp, pres, npre, n_grad, 0, wgs, bytes, __func__))
        return -1;
    if (ncomp == 0) return 0;
    if (!g || !comps_dev || !pres_dev || !w32 || !report || !scratch || (uintptr_t)scratch % 16) {
        kf_report_error("kf_ng_conv_apply: null or misaligned buffer (scratch 16 bytes)");
        return -1;
    }
    k_ngc_final<<<(unsigned)wgs[6], kThreads, 0, kf_stream()>>>(g, comps_dev, ncomp, pres_dev, w32, report, scratch);
    return ng_launched(__func__);
}
