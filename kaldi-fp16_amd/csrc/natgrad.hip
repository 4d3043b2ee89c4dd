// natgrad.hip — natural-gradient preconditioning of the weight gradients (include/kf_ops.h
// kf_ng_*): the online method of Povey, Zhang and Khudanpur (Kaldi's NG-SGD),
// batched over a table of preconditioners.
//
//   k_ng_init      the default initial state
//   k_ng_trx_*     tr(X X^T) of a KfOperand: the source rows' sums of squares times their
//                  multiplicities under the splice, workgroup partials in double, summed in order
//   k_ng_scales    gamma per preconditioner and the report
//   k_ng_apply<P>  four passes over the gradient segments:
//                  1 P = W_in G (partials per 256 rows of G) and 2 G <- g (G - W_in^T P) in double on
//                  the vector unit, 3 Q = G W_out^T and 4 G <- g' (G - Q W_out) on the exact f32-input MFMA
//   k_ng_state     one workgroup per preconditioner: K = J J^T and Z in double in LDS, cyclic Jacobi sweeps
//                  (round-robin pairs, so a round's rotations are disjoint), eigenvalues sorted
//                  and floored, rho', d', W'
// A workgroup finds its table entry by a scan of the table (a few dozen entries) in the order
// the host sized the launch by.
//
// Every sum runs in a fixed order (the MFMA's k-ordered fma chain, per-thread loops in index
// order, waves by shuffles, waves through LDS in wave order), so two runs give the same bits.
#include "kf_common.h"
#include "../../include/kf_ops.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;        // init, trx, apply: 4 waves
constexpr int kStateThreads = 1024;  // k_ng_state
constexpr int kMaxR = KF_NG_MAX_RANK;
constexpr int kTrxRows = 64;         // source rows per workgroup of k_ng_trx_part
constexpr int kPChunk = 256;         // rows of G per partial product of pass 1
constexpr int kSweeps = 30;          // Jacobi sweeps at most (double converges in under 12)
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

// ---------------------------------------------------------------- init
__global__ __launch_bounds__(kThreads) void k_ng_init(const KfNgPre *__restrict__ pres, KfNgOpts o,
                                                      float *__restrict__ w32, h16 *__restrict__ w16,
                                                      double *__restrict__ sc) {
    const KfNgPre p = pres[blockIdx.x];
    const int D = p.D, R = p.R, Rp = ng_rp(R), ldh = ng_ldh(D);
    const double eps = (double)o.epsilon, alpha = (double)o.alpha;
    const double beta = eps * (1.0 + alpha) + alpha * (R * eps) / D;
    const double se = sqrt(1.0 / (beta / eps + 1.0));
    for (long long idx = threadIdx.x; idx < (long long)Rp * D; idx += kThreads) {
        const int i = (int)(idx / D), j = (int)(idx - (long long)i * D);
        float v = 0.f;
        if (i < R && j % R == i) v = (float)(se / sqrt((double)((D - i + R - 1) / R)));  // the row's unit length
        w32[p.w_off + idx] = v;
        w16[p.h_off + (long long)i * ldh + j] = f2h(v);
        if (j == D - 1) w16[p.h_off + (long long)Rp * ldh + i] = f2h(v);
    }
    for (int idx = threadIdx.x; idx < Rp * (ldh - D); idx += kThreads)  // the rows' padding to ldh
        w16[p.h_off + (long long)(idx / (ldh - D)) * ldh + D + idx % (ldh - D)] = f2h(0.f);
    for (int i = threadIdx.x; i < Rp + 2; i += kThreads)
        sc[p.s_off + i] = i == 0 ? eps : i == 1 ? 0.0 : (i - 2 < R ? eps : 0.0);
}

// ---------------------------------------------------------------- trX
// how many (logical row, part) pairs of the operand read source row st (hout = 1)
__device__ long long ng_mult(const KfOperand &o, int st) {
    long long m = 0;
    for (int p = 0; p < o.nparts; ++p) {
        const int et = o.edge_t[p], dt = o.dt[p];
        const bool edge = et >= 0 && et < o.nrows;
        if (edge && st == o.edge_row[p]) m += 1;
        if (st >= o.T) continue;
        const long long t = (long long)st - dt;
        if (t >= 0 && t < o.nrows && !(edge && t == et)) m += 1;
        if (o.tpolicy == KF_CLAMP) {
            if (st == 0) {  // rows t < -dt fall below the first source row
                const long long cnt = -dt < 0 ? 0 : (-dt > o.nrows ? o.nrows : -dt);
                m += cnt - (edge && et < cnt ? 1 : 0);
            }
            if (st == o.T - 1) {  // rows t >= T - dt fall past the last
                long long lo = (long long)o.T - dt;
                lo = lo < 0 ? 0 : (lo > o.nrows ? o.nrows : lo);
                m += o.nrows - lo - (edge && et >= lo ? 1 : 0);
            }
        }
    }
    return m;
}

__global__ __launch_bounds__(kThreads) void k_ng_trx_part(KfOperand o, int tsrc, double *__restrict__ part) {
    __shared__ double sh[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const h16 *base = (const h16 *)o.base;
    double acc = 0.0;
    for (int i = wave; i < kTrxRows; i += kThreads / 64) {
        const int st = blockIdx.x * kTrxRows + i;
        if (st >= tsrc) break;
        const long long m = ng_mult(o, st);  // the same in the whole wave
        if (m == 0) continue;                // a row nothing reads is not read here either
        const h16 *row = base + (long long)st * o.ld;
        float s = 0.f;  // squares of fp16 values are exact in fp32
        for (int k = lane; k < o.part_width; k += 64) {
            const float v = h2f(row[k]);
            s += v * v;
        }
        acc += (double)m * (double)s;
    }
    acc = wave_sum(acc);
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(kThreads) void k_ng_trx_sum(const double *__restrict__ part, int nb, double add,
                                                         float nrows, float *__restrict__ out) {
    __shared__ double sh[kThreads / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += kThreads) s += part[i];
    s = block_sum_all(s, sh, kThreads / 64);
    if (threadIdx.x == 0) {
        out[0] = (float)(s + add);
        out[1] = nrows;
    }
}

// ---------------------------------------------------------------- scales
struct NgCoef {
    double eta, a, b;  // a = eta / N, b = 1 - eta
};
__device__ __forceinline__ NgCoef ng_coef(const KfNgOpts &o, double N) {
    NgCoef c;
    c.eta = 1.0 - exp(-N / (double)o.num_samples_history);
    if (c.eta > 0.9) c.eta = 0.9;
    c.a = c.eta / N;
    c.b = 1.0 - c.eta;
    return c;
}

__global__ __launch_bounds__(128) void k_ng_scales(const KfNgPre *__restrict__ pres, KfNgOpts o,
                                                   const double *__restrict__ sc, const float *__restrict__ stat,
                                                   float *__restrict__ report) {
    __shared__ double term[kMaxR], dsh[kMaxR];
    const KfNgPre p = pres[blockIdx.x];
    const int R = p.R, Rp = ng_rp(R), i = threadIdx.x;
    const double rho = sc[p.s_off];
    if (i < R) dsh[i] = sc[p.s_off + 2 + i];
    __syncthreads();
    double sumd = 0.0;
    for (int j = 0; j < R; ++j) sumd += dsh[j];
    const double beta = rho * (1.0 + (double)o.alpha) + (double)o.alpha * sumd / p.D;
    if (i < R) {
        const double e = 1.0 / (beta / dsh[i] + 1.0);
        term[i] = (2.0 - e) * (double)stat[p.st_off + KF_NG_STAT_L + (long long)i * Rp + i];
    }
    __syncthreads();
    if (i == 0) {
        const double trx = (double)stat[p.st_off];
        double sub = 0.0;
        for (int j = 0; j < R; ++j) sub += term[j];
        const double trh = trx - sub;
        double gamma = 1.0;
        if (isfinite(trx) && isfinite(trh) && trx > 0.0 && trh > 0.0) gamma = sqrt(trx / trh);
        float *rep = report + (long long)KF_NG_REPORT * blockIdx.x;
        rep[0] = (float)gamma;
        rep[1] = (float)rho;
        rep[2] = (float)sumd;
        rep[3] = (float)sc[p.s_off + 1];
        rep[4] = rep[5] = rep[6] = rep[7] = 0.f;
    }
}

// ---------------------------------------------------------------- apply
__host__ __device__ inline int ng_din(const KfNgComp &c) { return c.K + (c.db_off >= 0 ? 1 : 0); }
__host__ __device__ inline int ng_colgroups(int N) { return (ng_up32(N) / 32 + 3) / 4; }
__host__ __device__ inline int ng_pchunks(int din) { return (din + kPChunk - 1) / kPChunk; }
// workgroups of one table entry in a pass
__host__ __device__ inline long long ng_apply_wgs(const KfNgComp &c, const KfNgPre *pres, int pass) {
    const int rt = ng_up32(ng_din(c)) / 32;
    switch (pass) {
    case 1: return c.pre_in >= 0 ? (long long)ng_colgroups(c.N) * ng_pchunks(ng_din(c)) * (ng_rp(pres[c.pre_in].R) / 32) : 0;
    case 2: return c.pre_in >= 0 ? (long long)rt * ng_colgroups(c.N) : 0;
    case 3: return c.pre_out >= 0 ? rt : 0;
    default: return c.pre_out >= 0 ? (long long)rt * ng_colgroups(c.N) : 0;
    }
}
// scratch of one entry, floats: the chunks' partial P [Rp_in x up32(N)] each, in double, then
// Q [up32(Din) x Rp_out]
__host__ __device__ inline long long ng_p_floats(const KfNgComp &c, const KfNgPre *pres) {
    return c.pre_in >= 0 ? 2ll * ng_pchunks(ng_din(c)) * ng_rp(pres[c.pre_in].R) * ng_up32(c.N) : 0;
}
__host__ __device__ inline long long ng_q_floats(const KfNgComp &c, const KfNgPre *pres) {
    return c.pre_out >= 0 ? (long long)ng_up32(ng_din(c)) * ng_rp(pres[c.pre_out].R) : 0;
}

// element (row, col) of G = [dW ; db]
__device__ __forceinline__ long long ng_gidx(const KfNgComp &c, int row, int col) {
    return row < c.K ? c.dw_off + (long long)row * c.N + col : c.db_off + col;
}

template <int PASS>
__global__ __launch_bounds__(kThreads) void k_ng_apply(float *__restrict__ g, const KfNgComp *__restrict__ comps,
                                                       int ncomp, const KfNgPre *__restrict__ pres,
                                                       const float *__restrict__ w32,
                                                       const float *__restrict__ report, float *__restrict__ scratch) {
    long long b = blockIdx.x, soff = 0;
    int m = 0;
    for (; m < ncomp; ++m) {
        const KfNgComp t = comps[m];
        const long long cnt = ng_apply_wgs(t, pres, PASS);
        if (b < cnt) break;
        b -= cnt;
        soff += ng_p_floats(t, pres) + ng_q_floats(t, pres);
    }
    if (m == ncomp) return;  // the same in every thread
    const KfNgComp c = comps[m];
    const int Din = ng_din(c), N = c.N, Np = ng_up32(N);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    float *P = scratch + soff;
    float *Q = P + ng_p_floats(c, pres);
    if (PASS == 1) {
        // P[chunk] = W_in G over one chunk of Din, in double on the vector unit (as pass 2: P is
        // what G is cancelled against). A thread owns one column and 16 ranks of the workgroup's
        // 32 ranks x 128 columns; the chunks are summed in chunk order by pass 2.
        const KfNgPre pi = pres[c.pre_in];
        const int Rp = ng_rp(pi.R), ngr = ng_colgroups(N), nch = ng_pchunks(Din);
        const int n = (int)(b % ngr) * 128 + (threadIdx.x & 127), ch = (int)((b / ngr) % nch);
        const int rb = (int)(b / ((long long)ngr * nch)) * 32 + (threadIdx.x >> 7) * 16;
        if (n >= Np) return;
        const int k0 = ch * kPChunk, k1 = k0 + kPChunk < Din ? k0 + kPChunk : Din;
        const float *W = w32 + pi.w_off + (long long)rb * Din;
        double acc[16];
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0;
        if (n < N) {
            for (int k = k0; k < k1; ++k) {
                const double gk = (double)g[ng_gidx(c, k, n)];
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) acc[rr] += (double)W[(long long)rr * Din + k] * gk;
            }
        }
        double *Pc = (double *)P + (long long)ch * Rp * Np;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) Pc[(long long)(rb + rr) * Np + n] = acc[rr];
    } else if (PASS == 2) {
        // G <- gamma (G - W_in^T P) in double on the vector unit, in place (element-wise): where
        // gamma is large the result is a small difference of G and W^T P, and an fp32 chain over
        // the rank loses gamma times its rounding there (1.1e-5 relative at gamma 24, measured).
        // A thread owns one column and 16 rows of the workgroup's 32 x 128 block of G.
        const KfNgPre pi = pres[c.pre_in];
        const int Rp = ng_rp(pi.R), ngr = ng_colgroups(N), nch = ng_pchunks(Din);
        const int n = (int)(b % ngr) * 128 + (threadIdx.x & 127), ib = (int)(b / ngr) * 32 + (threadIdx.x >> 7) * 16;
        if (n >= N) return;
        const float *W = w32 + pi.w_off;
        const long long pstride = (long long)Rp * Np;
        double acc[16];
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) acc[ii] = ib + ii < Din ? (double)g[ng_gidx(c, ib + ii, n)] : 0.0;
        for (int k = 0; k < Rp; ++k) {
            double pk = 0.0;  // the chunks in chunk order
            for (int q = 0; q < nch; ++q) pk += ((const double *)P)[q * pstride + (long long)k * Np + n];
#pragma unroll
            for (int ii = 0; ii < 16; ++ii)
                if (ib + ii < Din) acc[ii] -= (double)W[(long long)k * Din + ib + ii] * pk;
        }
        double scale = (double)report[(long long)KF_NG_REPORT * c.pre_in];
        if (c.pre_out >= 0) scale *= (double)report[(long long)KF_NG_REPORT * c.pre_out];
#pragma unroll
        for (int ii = 0; ii < 16; ++ii)
            if (ib + ii < Din) g[ng_gidx(c, ib + ii, n)] = (float)(acc[ii] * scale);
    } else if (PASS == 4) {  // a 32 x 32 tile of G per wave, in place (element-wise)
        const int ngr = ng_colgroups(N), i0 = (int)(b / ngr) * 32, n0 = ((int)(b % ngr) * 4 + wave) * 32;
        if (n0 >= N) return;
        const KfNgPre po = pres[c.pre_out];
        const int Rp = ng_rp(po.R);
        const float *W = w32 + po.w_off;
        const bool ncol = n0 + r < N;
        const f32x16 acc = ng_tile(
            Rp, [&](int i, int k) { return Q[(long long)(i0 + i) * Rp + k]; },
            [&](int k, int j) { return ncol ? W[(long long)k * N + n0 + j] : 0.f; });
        const float scale = c.pre_in >= 0 ? 1.f : report[(long long)KF_NG_REPORT * c.pre_out];
        if (ncol) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = i0 + ng_drow(q, h);
                if (row < Din) {
                    const long long at = ng_gidx(c, row, n0 + r);
                    g[at] = (g[at] - acc[q]) * scale;
                }
            }
        }
    } else {  // PASS 3: Q[row tile b][rank tile wave] = G W_out^T over all of N
        const KfNgPre po = pres[c.pre_out];
        const int Rp = ng_rp(po.R), i0 = (int)b * 32;
        if (wave >= Rp / 32) return;
        const float *W = w32 + po.w_off + (long long)wave * 32 * N;
        const bool row = i0 + r < Din;
        const f32x16 acc = ng_tile(
            N, [&](int i, int k) { return row ? g[ng_gidx(c, i0 + i, k)] : 0.f; },
            [&](int k, int j) { return W[(long long)j * N + k]; });
#pragma unroll
        for (int q = 0; q < 16; ++q) Q[(long long)(i0 + ng_drow(q, h)) * Rp + wave * 32 + r] = acc[q];
    }
}

// ---------------------------------------------------------------- state
// round-robin pairing of n2 (even) players: in round r, slot 0 pairs n2 - 1 with r, slot i the
// players (r + i) and (r - i) modulo n2 - 1; every pair meets once per n2 - 1 rounds
__device__ __forceinline__ void ng_pair(int n2, int round, int slot, int &p, int &q) {
    const int m = n2 - 1;
    int a, b;
    if (slot == 0) {
        a = m;
        b = round;
    } else {
        a = (round + slot) % m;
        b = (round - slot + m) % m;
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

__global__ __launch_bounds__(kStateThreads) void k_ng_state(const KfNgPre *__restrict__ pres, KfNgOpts o,
                                                            int update, float *__restrict__ w32,
                                                            h16 *__restrict__ w16, double *__restrict__ sc,
                                                            const float *__restrict__ stat,
                                                            float *__restrict__ scratch, float *__restrict__ report) {
    extern __shared__ __attribute__((aligned(16))) double lds[];  // Z [R x R], U [R x R]
    __shared__ double dsh[kMaxR], fsh[kMaxR], drsh[kMaxR], cval[kMaxR], ssh[kMaxR], dnew[kMaxR], gsh[kMaxR];
    __shared__ double rc[kMaxR / 2 + 1], rs[kMaxR / 2 + 1], red[kStateThreads / 64];
    __shared__ double sh_rho1;
    __shared__ int perm[kMaxR], rankof[kMaxR], bad, done;
    const int tid = threadIdx.x;
    const KfNgPre p = pres[blockIdx.x];
    double *tcount = sc + p.s_off + 1;
    if (!update) {  // the same in every thread
        if (tid == 0) *tcount += 1.0;
        return;
    }
    const int D = p.D, R = p.R, Rp = ng_rp(R);
    double *Z = lds, *U = lds + R * R;
    const float *st = stat + p.st_off;
    const float *Lm = st + KF_NG_STAT_L, *JT = st + KF_NG_STAT_JT(Rp);
    // this preconditioner's W' before it is committed: the scratch regions follow the table
    long long woff = 0;
    for (int q = 0; q < (int)blockIdx.x; ++q) woff += (long long)pres[q].R * pres[q].D;
    float *Wt = scratch + woff;
    float *W = w32 + p.w_off;
    h16 *Wh = w16 + p.h_off;
    const int ldh = ng_ldh(p.D);

    const double rho = sc[p.s_off], trx = (double)st[0], N = (double)st[1];
    const double eps = (double)o.epsilon, alpha = (double)o.alpha;
    if (tid == 0) {
        bad = !(isfinite(trx) && isfinite(N) && N >= 1.0 && isfinite(rho) && rho > 0.0);
        done = 0;
    }
    if (tid < R) dsh[tid] = sc[p.s_off + 2 + tid];
    __syncthreads();
    double sumd = 0.0;
    for (int j = 0; j < R; ++j) sumd += dsh[j];
    const NgCoef cf = ng_coef(o, N);
    const double beta = rho * (1.0 + alpha) + alpha * sumd / D;
    if (tid < R) {
        const double e = 1.0 / (beta / dsh[tid] + 1.0);
        fsh[tid] = 1.0 / sqrt(e);
        drsh[tid] = dsh[tid] + rho;
        if (!isfinite(fsh[tid])) bad = 1;
    }
    __syncthreads();
    // K = J J^T in double from the fp32 JT, so that Z below is (a F J)(a F J)^T to double's
    // rounding whatever J's own error: the rows of R' then come out with unit length even where an
    // eigenvalue is 1e-12 of the largest. (From a K rounded to fp32 those rows were scaled by
    // noise / floor: W grew to 1e7 on the first update of a 3072-wide input.)
    for (int idx = tid; idx < R * R; idx += kStateThreads) {
        const int i = idx / R, j = idx - i * R;
        double acc = 0.0;
        for (int k = 0; k < D; ++k) acc += (double)JT[(long long)k * Rp + i] * (double)JT[(long long)k * Rp + j];
        Z[idx] = acc;
    }
    __syncthreads();
    // Z, symmetric by construction: (i, j) and (j, i) are the same expression
    for (int idx = tid; idx < R * R; idx += kStateThreads) {
        const int i = idx / R, j = idx - i * R;
        const double k = Z[idx];
        const double l = 0.5 * ((double)Lm[(long long)i * Rp + j] + (double)Lm[(long long)j * Rp + i]);
        const double ff = fsh[i] * fsh[j];
        double z = cf.a * cf.a * (ff * k) + cf.a * cf.b * ((drsh[i] + drsh[j]) * (ff * l));
        if (i == j) z += cf.b * cf.b * drsh[i] * drsh[i];
        if (!isfinite(z)) bad = 1;
        Z[idx] = z;
        U[idx] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    if (!bad) {  // the same in every thread
        const int n2 = R + (R & 1), np = n2 / 2;
        for (int sweep = 0; sweep < kSweeps; ++sweep) {
            double off = 0.0, all = 0.0;
            for (int idx = tid; idx < R * R; idx += kStateThreads) {
                const double z = Z[idx];
                all += z * z;
                if (idx / R != idx % R) off += z * z;
            }
            off = block_sum_all(off, red, kStateThreads / 64);
            all = block_sum_all(all, red, kStateThreads / 64);
            if (!(off > 1e-32 * all)) break;  // the same in every thread (also ends on a NaN)
            for (int round = 0; round < n2 - 1; ++round) {
                if (tid < np) {
                    int a, b;
                    ng_pair(n2, round, tid, a, b);
                    double c = 1.0, s = 0.0;
                    if (b < R) {
                        const double apq = Z[a * R + b];
                        if (apq != 0.0) {
                            const double tau = (Z[b * R + b] - Z[a * R + a]) / (2.0 * apq);
                            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                            c = 1.0 / sqrt(1.0 + t * t);
                            s = t * c;
                        }
                    }
                    rc[tid] = c;
                    rs[tid] = s;
                }
                __syncthreads();
                for (int idx = tid; idx < np * R; idx += kStateThreads) {  // rows a, b of J^T Z
                    const int slot = idx / R, k = idx - slot * R;
                    int a, b;
                    ng_pair(n2, round, slot, a, b);
                    if (b >= R) continue;
                    const double c = rc[slot], s = rs[slot], za = Z[a * R + k], zb = Z[b * R + k];
                    Z[a * R + k] = c * za - s * zb;
                    Z[b * R + k] = s * za + c * zb;
                }
                __syncthreads();
                for (int idx = tid; idx < np * R; idx += kStateThreads) {  // columns a, b of (.) J and of U J
                    const int slot = idx / R, k = idx - slot * R;
                    int a, b;
                    ng_pair(n2, round, slot, a, b);
                    if (b >= R) continue;
                    const double c = rc[slot], s = rs[slot];
                    const double za = Z[k * R + a], zb = Z[k * R + b], ua = U[k * R + a], ub = U[k * R + b];
                    Z[k * R + a] = c * za - s * zb;
                    Z[k * R + b] = s * za + c * zb;
                    U[k * R + a] = c * ua - s * ub;
                    U[k * R + b] = s * ua + c * ub;
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    // eigenvalues floored, descending (ties by index)
    const double floor_c = (rho * cf.b) * (rho * cf.b);
    if (tid < R) {
        double c = Z[tid * R + tid];
        if (!isfinite(c)) bad = 1;
        if (!(c > floor_c)) c = floor_c;
        cval[tid] = c;
    }
    __syncthreads();
    if (tid < R) {
        int rank = 0;
        for (int j = 0; j < R; ++j) rank += (cval[j] > cval[tid] || (cval[j] == cval[tid] && j < tid)) ? 1 : 0;
        rankof[tid] = rank;
        perm[rank] = tid;
        ssh[rank] = sqrt(cval[tid]);
    }
    __syncthreads();
    if (tid == 0) {
        double sums = 0.0;
        for (int j = 0; j < R; ++j) sums += ssh[j];
        double rho1 = (cf.a * trx + cf.b * ((double)D * rho + sumd) - sums) / (double)(D - R);
        if (!isfinite(rho1)) bad = 1;
        if (!(rho1 > eps)) rho1 = eps;
        const double top = o.delta * (ssh[0] - rho1);
        double sumd1 = 0.0;
        for (int j = 0; j < R; ++j) {
            double d = ssh[j] - rho1;
            if (d < eps) d = eps;
            if (d < top) d = top;
            dnew[j] = d;
            sumd1 += d;
        }
        const double beta1 = rho1 * (1.0 + alpha) + alpha * sumd1 / D;
        for (int j = 0; j < R; ++j) {
            const double e1 = 1.0 / (beta1 / dnew[j] + 1.0);
            gsh[j] = sqrt(e1) / ssh[j];  // row j of W' = gsh[j] * (column perm[j] of U)^T (...)
            if (!isfinite(gsh[j]) || !isfinite(dnew[j])) bad = 1;
        }
        sh_rho1 = rho1;
    }
    __syncthreads();
    // the coefficients of JT and of W per (source row j, eigenvector i), in place of Z and U
    for (int idx = tid; idx < R * R; idx += kStateThreads) {
        const int j = idx / R, i = idx - j * R;
        const double u = U[idx] * gsh[rankof[i]];
        Z[idx] = u * (cf.a * fsh[j]);
        U[idx] = u * (cf.b * drsh[j] * fsh[j]);
    }
    __syncthreads();
    // W' [R x D] into scratch: thread k owns column k, 16 rows at a time
    int mybad = 0;
    if (!bad) {
        for (int k = tid; k < D; k += kStateThreads) {
            for (int r0 = 0; r0 < R; r0 += 16) {
                double acc[16];
                int col[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    acc[c] = 0.0;
                    col[c] = perm[r0 + c < R ? r0 + c : R - 1];
                }
                for (int j = 0; j < R; ++j) {
                    const double jv = (double)JT[(long long)k * Rp + j], wv = (double)W[(long long)j * D + k];
#pragma unroll
                    for (int c = 0; c < 16; ++c) acc[c] += Z[j * R + col[c]] * jv + U[j * R + col[c]] * wv;
                }
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    if (r0 + c < R) {
                        const float v = (float)acc[c];
                        if (!isfinite(v)) mybad = 1;
                        Wt[(long long)(r0 + c) * D + k] = v;
                    }
                }
            }
        }
    }
    if (mybad) bad = 1;
    __syncthreads();
    if (!bad) {  // commit: thread k copies the column it wrote
        for (int k = tid; k < D; k += kStateThreads) {
            for (int r = 0; r < R; ++r) {
                const float v = Wt[(long long)r * D + k];
                W[(long long)r * D + k] = v;
                Wh[(long long)r * ldh + k] = f2h(v);
                if (k == D - 1) Wh[(long long)Rp * ldh + r] = f2h(v);
            }
        }
        if (tid < R) sc[p.s_off + 2 + tid] = dnew[tid];
        if (tid == 0) sc[p.s_off] = sh_rho1;
    }
    if (tid == 0) {
        *tcount += 1.0;
        if (bad) report[(long long)KF_NG_REPORT * blockIdx.x + 4] = 1.f;
    }
}

// ---------------------------------------------------------------- host side
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

bool ng_check_comps(const KfNgComp *comps, int ncomp, const KfNgPre *pres, int npre, long long n_grad,
                    long long wgs[5], long long &floats, const char *who) {
    floats = 0;
    for (int q = 0; q < 5; ++q) wgs[q] = 0;
    if (ncomp < 0 || (ncomp > 0 && !comps)) {
        kf_report_error("%s: bad component table (%d entries)", who, ncomp);
        return false;
    }
    for (int m = 0; m < ncomp; ++m) {
        const KfNgComp &c = comps[m];
        const bool in_ok = c.pre_in < 0 || (c.pre_in < npre && pres[c.pre_in].D == ng_din(c));
        const bool out_ok = c.pre_out < 0 || (c.pre_out < npre && pres[c.pre_out].D == c.N);
        if (c.K < 1 || c.N < 1 || !in_ok || !out_ok) {
            kf_report_error("%s: component %d (%d x %d) does not match its preconditioners", who, m, c.K, c.N);
            return false;
        }
        if (c.dw_off < 0 || (n_grad >= 0 && (c.dw_off + (long long)c.K * c.N > n_grad ||
                                             (c.db_off >= 0 && c.db_off + c.N > n_grad)))) {
            kf_report_error("%s: component %d lies outside the %lld gradient elements", who, m, n_grad);
            return false;
        }
        for (int q = 1; q <= 4; ++q) wgs[q] += ng_apply_wgs(c, pres, q);
        floats += ng_p_floats(c, pres) + ng_q_floats(c, pres);
    }
    for (int q = 1; q <= 4; ++q)
        if (wgs[q] > 0x7fffffffll) {
            kf_report_error("%s: more than 2^31 workgroups", who);
            return false;
        }
    return true;
}

int ng_launched(const char *who) {
    return hipGetLastError() == hipSuccess ? 0 : (kf_report_error("%s: launch failed", who), -1);
}

}  // namespace

extern "C" void kf_ng_default_opts(KfNgOpts *o) {
    if (!o) return;
    o->rank_in = 20;
    o->rank_out = 80;
    o->update_period = 4;
    o->num_samples_history = 2000.f;
    o->alpha = 4.f;
    o->epsilon = 1e-10f;
    o->delta = 5e-4f;
}

extern "C" int kf_ng_init(const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const KfNgOpts *opts, float *w32,
                          void *w16, double *sc) {
    kf_take_pending(__func__);
    if (!ng_check_pres(pres, npre, __func__) || !ng_check_opts(opts, __func__)) return -1;
    if (npre == 0) return 0;
    if (!pres_dev || !w32 || !w16 || !sc) {
        kf_report_error("kf_ng_init: null buffer");
        return -1;
    }
    k_ng_init<<<(unsigned)npre, kThreads, 0, kf_stream()>>>(pres_dev, *opts, w32, (h16 *)w16, sc);
    return ng_launched(__func__);
}

extern "C" int kf_ng_trx(const KfOperand *op, int ones, float *out) {
    kf_take_pending(__func__);
    if (!op || !out || !op->base) {
        kf_report_error("kf_ng_trx: null argument");
        return -1;
    }
    const KfOperand &o = *op;
    bool ok = o.fmt == KF_FMT_FP16 && !o.mask && o.hout == 1 && o.hsrc == 1 && o.hdiv == 1 && o.tmul == 0 && o.t0 == 0 &&
              o.nparts >= 1 && o.nparts <= KF_MAX_PARTS && o.part_width >= 1 && o.ncols == o.nparts * o.part_width &&
              o.nrows >= 1 && o.T >= 1 && o.ld >= o.part_width && (o.tpolicy == KF_ZERO || o.tpolicy == KF_CLAMP);
    int tsrc = o.T;
    for (int p = 0; ok && p < o.nparts; ++p) {
        if (o.dh[p] != 0) ok = false;
        if (o.edge_t[p] >= 0) {
            if (o.edge_row[p] < 0) ok = false;
            if (o.edge_row[p] >= tsrc) tsrc = o.edge_row[p] + 1;
        }
    }
    if (!ok) {
        kf_report_error("kf_ng_trx: only fp16 operands with hout = 1, no mask, no time stride and no height offsets");
        return -1;
    }
    const int nb = (tsrc + kTrxRows - 1) / kTrxRows;
    double *part = (double *)kf_workspace_stream((size_t)nb * sizeof(double));
    if (!part) {
        kf_report_error("kf_ng_trx: no workspace");
        return -1;
    }
    k_ng_trx_part<<<(unsigned)nb, kThreads, 0, kf_stream()>>>(o, tsrc, part);
    k_ng_trx_sum<<<1, kThreads, 0, kf_stream()>>>(part, nb, ones ? (double)o.nrows : 0.0, (float)o.nrows, out);
    return ng_launched(__func__);
}

extern "C" int kf_ng_scales(const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const KfNgOpts *opts,
                            const double *sc, const float *stat, float *report) {
    kf_take_pending(__func__);
    if (!ng_check_pres(pres, npre, __func__) || !ng_check_opts(opts, __func__)) return -1;
    if (npre == 0) return 0;
    if (!pres_dev || !sc || !stat || !report) {
        kf_report_error("kf_ng_scales: null buffer");
        return -1;
    }
    k_ng_scales<<<(unsigned)npre, 128, 0, kf_stream()>>>(pres_dev, *opts, sc, stat, report);
    return ng_launched(__func__);
}

extern "C" long long kf_ng_apply_scratch_bytes(const KfNgComp *comps, int ncomp, const KfNgPre *pres, int npre) {
    long long wgs[5], floats;
    if (!ng_check_pres(pres, npre, __func__) || !ng_check_comps(comps, ncomp, pres, npre, -1, wgs, floats, __func__))
        return -1;
    return (long long)ng_align((size_t)floats * 4);
}

extern "C" int kf_ng_apply(float *g, long long n_grad, const KfNgComp *comps, const KfNgComp *comps_dev, int ncomp,
                           const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const float *w32,
                           const float *report, void *scratch) {
    kf_take_pending(__func__);
    long long wgs[5], floats;
    if (n_grad < 0) {
        kf_report_error("kf_ng_apply: bad arguments");
        return -1;
    }
    if (!ng_check_pres(pres, npre, __func__) || !ng_check_comps(comps, ncomp, pres, npre, n_grad, wgs, floats, __func__))
        return -1;
    if (wgs[1] + wgs[3] == 0) return 0;  // nothing is preconditioned: no launch
    if (!g || !comps_dev || !pres_dev || !w32 || !report || !scratch || (uintptr_t)scratch % 16) {
        kf_report_error("kf_ng_apply: null or misaligned buffer (scratch 16 bytes)");
        return -1;
    }
    float *s = (float *)scratch;
    hipStream_t st = kf_stream();
    if (wgs[1]) {
        k_ng_apply<1><<<(unsigned)wgs[1], kThreads, 0, st>>>(g, comps_dev, ncomp, pres_dev, w32, report, s);
        k_ng_apply<2><<<(unsigned)wgs[2], kThreads, 0, st>>>(g, comps_dev, ncomp, pres_dev, w32, report, s);
    }
    if (wgs[3]) {
        k_ng_apply<3><<<(unsigned)wgs[3], kThreads, 0, st>>>(g, comps_dev, ncomp, pres_dev, w32, report, s);
        k_ng_apply<4><<<(unsigned)wgs[4], kThreads, 0, st>>>(g, comps_dev, ncomp, pres_dev, w32, report, s);
    }
    return ng_launched(__func__);
}

extern "C" long long kf_ng_state_scratch_bytes(const KfNgPre *pres, int npre) {
    if (!ng_check_pres(pres, npre, __func__)) return -1;
    long long floats = 0;
    for (int m = 0; m < npre; ++m) floats += (long long)pres[m].R * pres[m].D;
    return (long long)ng_align((size_t)floats * 4);
}

extern "C" int kf_ng_state(const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const KfNgOpts *opts, int update,
                           float *w32, void *w16, double *sc, const float *stat, void *scratch, float *report) {
    kf_take_pending(__func__);
    if (!ng_check_pres(pres, npre, __func__) || !ng_check_opts(opts, __func__)) return -1;
    if (npre == 0) return 0;
    if (!pres_dev || !w32 || !w16 || !sc || !stat || !scratch || !report || (uintptr_t)scratch % 16) {
        kf_report_error("kf_ng_state: null or misaligned buffer (scratch 16 bytes)");
        return -1;
    }
    int maxr = 0;
    for (int m = 0; m < npre; ++m) maxr = pres[m].R > maxr ? pres[m].R : maxr;
    const size_t lds = update ? (size_t)2 * maxr * maxr * sizeof(double) : 0;
    static size_t lds_allowed = 0;  // the largest dynamic LDS size asked of the runtime so far
    if (lds > 48 * 1024 && lds > lds_allowed) {
        if (hipFuncSetAttribute((const void *)k_ng_state, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess) {
            (void)hipGetLastError();
            kf_report_error("kf_ng_state: %zu bytes of LDS refused", lds);
            return -1;
        }
        lds_allowed = lds;
    }
    k_ng_state<<<(unsigned)npre, kStateThreads, lds, kf_stream()>>>(pres_dev, *opts, update, w32, (h16 *)w16, sc, stat,
                                                                    (float *)scratch, report);
    return ng_launched(__func__);
}
