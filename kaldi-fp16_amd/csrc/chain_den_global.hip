// chain_den_global.hip — the chain denominator with its state rows in device memory:
// the path for graphs the LDS-resident kernels of chain_den.hip refuse (more than 4096 pdfs, 8192
// states or more), chosen by kf_den_graph_create_rows. The mathematics is chain_den.hip's; the
// organisation is Kaldi's: one launch per frame and direction, each over all sequences and all
// state rows, so the frame-to-frame dependence is the stream's launch order and no workgroup
// ever waits on another. No atomics: per-row sums run in table order, the per-frame sums are
// per-workgroup partials in a fixed layout that the next launch re-sums in index order.
//
// Rows interleave the NQ = min(64, pow2 >= nseq) sequences of a group, q fastest: row[t][state][q].
// A wave works on 64 / NQ table rows x NQ sequences; the NQ lanes of a row load NQ consecutive
// records with one coalesced load and pass them round by lane shuffles, so a record is fetched
// once for all NQ sequences and every alpha[src][.] / beta[dst][.] / e[pdf][.] gather is one
// contiguous 4 * NQ-byte segment. The per-row summation order is the table's, whatever NQ.
//   k_dg_stage   exp(clamp(x)) of the supervised rows, transposed through LDS to e[t][pdf][q]
//   k_dg_row0    alpha[0] = init
//   k_dg_rec     one frame of the forward (alpha) or backward (beta') recursion
//   k_dg_sums    the partials of every frame summed once for the posteriors; k_dg_lp: den_lp
//   k_dg_post    the posteriors of every (group, frame) by pdf rows, in place of e
//   k_dg_asm     normalisation, the objective assembly of k_den_post's product mode, fp16 rows
//   k_dg_stats   the per-sequence statistics, per-frame terms summed in frame order
#include "chain_den_global.h"

// ---- places in the workspace (every group's share scales with NQ) --------------------------------
__device__ __forceinline__ float *dg_alpha(const DgDev &g, const DgRun &r, int grp, int t) {
    return r.w.alpha + ((size_t)grp * (r.max_frames + 1) + t) * g.f.nrows * r.NQ;
}
__device__ __forceinline__ float *dg_beta(const DgDev &g, const DgRun &r, int grp, int t) {  // t >= 1
    return r.w.beta + ((size_t)grp * r.max_frames + (t - 1)) * g.b.nrows * r.NQ;
}
__device__ __forceinline__ float *dg_e(const DgDev &g, const DgRun &r, int grp, int t) {
    return r.w.e + ((size_t)grp * r.max_frames + t) * g.P * r.NQ;
}
__device__ __forceinline__ float *dg_part(float *base, const DgRun &r, int grp, int t, int rows) {
    return base + ((size_t)grp * rows + t) * DG_MAXWG * r.NQ;
}
__device__ __forceinline__ float *dg_sum(float *base, const DgRun &r, int grp, int t) {
    return base + ((size_t)grp * (r.max_frames + 1) + t) * r.NQ;
}

// The n per-workgroup partials part[i][q] of a frame summed in a fixed order for this thread's
// q = tid % NQ: up to 16 column sums over i = j, j + J, ..., then those in j order. Every thread
// of the block calls it (two barriers); lds: 16 x 64 floats, free again on return.
__device__ __forceinline__ float dg_resum(const float *part, int n, int NQ, float *lds) {
    const int tid = threadIdx.x, q = tid % NQ, j = tid / NQ;
    const int J = min(16, (int)blockDim.x / NQ);
    if (j < J) {
        float s = 0.f;
        for (int i = j; i < n; i += J) s += part[(size_t)i * NQ + q];
        lds[j * 64 + q] = s;
    }
    __syncthreads();
    float s = 0.f;
    for (int jj = 0; jj < J; ++jj) s += lds[jj * 64 + q];
    __syncthreads();
    return s;
}

// The wave's per-sequence sums over its rows: across the 64 / NQ rows of a wave by butterflies,
// across the block's waves in wave order; thread q < NQ stores the workgroup's partial.
template <int NQ>
__device__ __forceinline__ void dg_store_partial(float psum, float *red, float *out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o >= NQ; o >>= 1) psum += __shfl_xor(psum, o, 64);
    if (lane < NQ) red[wave * 64 + lane] = psum;
    __syncthreads();
    if (tid < NQ) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < DG_WAVES; ++w) s += red[w * 64 + tid];
        out[(size_t)blockIdx.x * NQ + tid] = s;
    }
}

// Sum over the records of table row `row` for this lane's sequence, in table order. The NQ lanes
// of the row load NQ consecutive records at once and hand them round; `load(on, f1, f2, a, b)`
// gathers the two operands of a record (predicated), `mul(a, b, tp, ti)` is its term. Up to 8
// records' gathers are in flight before the first product.
template <int NQ, bool TI, class L, class M>
__device__ __forceinline__ float dg_row_sum(const DgTabDev &tb, int row, int lane, L load, M mul) {
    constexpr int U = NQ < 8 ? NQ : 8;
    const int q = lane % NQ, sub0 = lane - q;
    const int b0 = tb.rowptr[row], len = tb.rowptr[row + 1] - b0;
    const int kmax = __shfl(len, 0, 64);  // rows are sorted by degree: the wave's first is its longest
    float acc = 0.f;
    for (int k0 = 0; k0 < kmax; k0 += NQ) {
        uint2 rc = make_uint2(0u, 0u);
        float ti = 0.f;
        if (k0 + q < len) {
            rc = tb.rec[b0 + k0 + q];
            if (TI) ti = tb.ti[b0 + k0 + q];
        }
        const int n = min(NQ, kmax - k0);
        for (int i0 = 0; i0 < n; i0 += U) {
            unsigned rx[U];
            float tp[U], tv[U], a[U], b[U];
            bool on[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int from = sub0 + i0 + u;
                rx[u] = NQ == 1 ? rc.x : (unsigned)__shfl((int)rc.x, from, 64);
                tp[u] = NQ == 1 ? __uint_as_float(rc.y) : __shfl(__uint_as_float(rc.y), from, 64);
                tv[u] = !TI ? 0.f : NQ == 1 ? ti : __shfl(ti, from, 64);
                on[u] = k0 + i0 + u < len;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) load(on[u], (int)(rx[u] & 0xFFFF), (int)(rx[u] >> 16), a[u], b[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (on[u]) acc += mul(a[u], b[u], tp[u], tv[u]);
        }
    }
    return acc;
}

// ---- staging ---------------------------------------------------------------------------------------
// exp(clamp(x)) of frame t of the group's sequences, 64 pdfs x NQ sequences per block through a
// padded LDS tile: the reads run along a matrix row, the writes along q. 0 past a sequence's last
// frame and for absent sequences, so the recursions read e without a frame test.
__global__ __launch_bounds__(256) void k_dg_stage(const DgDev g, const DgRun r) {
    __shared__ float tile[64 * 65];
    const int tid = threadIdx.x, NQ = r.NQ, P = g.P;
    const int p0 = blockIdx.x * 64, t = blockIdx.y, grp = blockIdx.z;
    const h16 *nnet = reinterpret_cast<const h16 *>(r.nnet);
    for (int qq = tid >> 6; qq < NQ; qq += 4) {
        const int seq = grp * NQ + qq, p = p0 + (tid & 63);
        const int T = seq < r.nseq ? r.frames[seq] : 0;
        float v = 0.f;
        if (t < T && p < P) {
            const float x = (float)nnet[(r.row0[seq] + (long long)t * r.stride) * r.ld + p];
            v = expf(fmaxf(-30.0f, fminf(30.0f, x)));  // kernel_apply_exp
        }
        tile[qq * 65 + (tid & 63)] = v;
    }
    __syncthreads();
    float *e = dg_e(g, r, grp, t);
    for (int idx = tid; idx < 64 * NQ; idx += 256) {
        const int q = idx % NQ, pp = idx / NQ;
        if (p0 + pp < P) e[(size_t)(p0 + pp) * NQ + q] = tile[q * 65 + pp];
    }
}

// alpha[0][pos][q] = init of the state at pos (AlphaFirstFrame), every group
__global__ void k_dg_row0(const DgDev g, const DgRun r) {
    const int n = g.f.nrows * r.NQ, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dg_alpha(g, r, blockIdx.y, 0)[i] = g.f.initp[i / r.NQ];
}

// ---- one frame of a recursion ----------------------------------------------------------------------
// DIR 0: alpha[t+1][r] = sum_arcs alpha'[t][src] tp e[t][pdf] / asum[t] over the rows (destination
//        states) of the f table, alpha'[t] = alpha[t] + asum[t] leaky init: the second term rides
//        in the records as ti = tp init[src], so the gather stays one segment per operand.
// DIR 1: beta'[t][r] = sum_arcs tp e[t][pdf] beta[t+1][dst] / nrm[t+1] over the rows (source states)
//        of the b table, beta[t+1] = beta'[t+1] + leaky nrm[t+1], nrm = <init, beta'>; a sequence
//        whose last frame is t starts from beta'[T] = 1, nrm[T] = sum(init) (den_bwd_body).
// The frame's scalar (asum[t] / nrm[t+1]) is the previous launch's partials, re-summed by every
// workgroup; this launch's rows leave theirs for the next. Rows go round the grid's waves
// cyclically: they are sorted by degree, so every wave gets the same mix.
template <int NQ, int DIR>
__global__ __launch_bounds__(DG_THREADS) void k_dg_rec(const DgDev g, const DgRun r, int t) {
    __shared__ float red[DG_WAVES * 64];
    constexpr int R = 64 / NQ;
    const DgTabDev &tb = DIR ? g.b : g.f;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane % NQ, sub = lane / NQ, grp = blockIdx.y;
    const int seq = grp * NQ + q;
    const int T = seq < r.nseq ? r.frames[seq] : 0;
    const bool live = t < T, first = DIR && t + 1 == T;
    const int nwg = gridDim.x;
    float s;  // asum[t] or nrm[t+1]
    if (DIR) {
        s = t + 1 < r.Tm ? dg_resum(dg_part(r.w.bpart, r, grp, t + 1, r.max_frames + 1), nwg, NQ, red) : g.as0;
        if (first) s = g.as0;
    } else {
        s = t > 0 ? dg_resum(dg_part(r.w.apart, r, grp, t, r.max_frames + 1), nwg, NQ, red) : g.as0;
    }
    const float inv = s > 0.0f ? 1.0f / s : 1.0f, c = s * r.leaky;
    const float *vin = DIR ? (t + 1 < r.Tm ? dg_beta(g, r, grp, t + 1) : nullptr) : dg_alpha(g, r, grp, t);
    float *vout = DIR ? dg_beta(g, r, grp, t) : dg_alpha(g, r, grp, t + 1);
    const float *er = dg_e(g, r, grp, t);
    const int nrg = tb.nrows / R, W = nwg * DG_WAVES;
    float psum = 0.f;
    for (int rg = blockIdx.x * DG_WAVES + wave; rg < nrg; rg += W) {
        const int row = rg * R + sub;
        const float acc = dg_row_sum<NQ, DIR == 0>(
            tb, row, lane,
            [&](bool on, int f1, int f2, float &a, float &x) {
                on = on && live;
                a = DIR && first ? 1.0f : 0.0f;
                if (on && !(DIR && first)) a = vin[(size_t)f1 * NQ + q];
                x = on ? er[(size_t)f2 * NQ + q] : 0.0f;
            },
            [&](float a, float x, float tp, float ti) { return DIR ? tp * x * (a + c) : (a * tp + c * ti) * x; });
        const float v = acc * inv;  // padding rows have no records: 0
        if (live) vout[(size_t)row * NQ + q] = v;
        psum += DIR ? tb.initp[row] * v : v;
    }
    dg_store_partial<NQ>(psum, red, dg_part(DIR ? r.w.bpart : r.w.apart, r, grp, DIR ? t : t + 1, r.max_frames + 1));
}

// asum[t] and nrm[t] of every (group, frame) once, for the posteriors and den_lp
__global__ __launch_bounds__(DG_THREADS) void k_dg_sums(const DgDev g, const DgRun r, int nwg) {
    __shared__ float red[DG_WAVES * 64];
    const int t = blockIdx.x, grp = blockIdx.y, NQ = r.NQ, tid = threadIdx.x;
    const float a = t > 0 ? dg_resum(dg_part(r.w.apart, r, grp, t, r.max_frames + 1), nwg, NQ, red) : g.as0;
    const float b = t > 0 && t < r.Tm ? dg_resum(dg_part(r.w.bpart, r, grp, t, r.max_frames + 1), nwg, NQ, red) : g.as0;
    if (tid < NQ) {
        dg_sum(r.w.asum, r, grp, t)[tid] = a;
        dg_sum(r.w.bsum, r, grp, t)[tid] = b;
    }
}

// total_prob = sum(alpha'[T]) = asum[T] (1 + leaky sum(init)); den_lp = log(total) + sum_{t<T} log(asum[t])
__global__ void k_dg_lp(const DgDev g, const DgRun r) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= r.nseq) return;
    const int grp = seq / r.NQ, q = seq % r.NQ, T = r.frames[seq];
    float total = 0.f, lp = 0.f;
    if (T > 0) {
        const float aT = dg_sum(r.w.asum, r, grp, T)[q];
        total = aT + aT * r.leaky * g.as0;
        double lc = 0.0;
        for (int t = 0; t < T; ++t) {
            const float a = dg_sum(r.w.asum, r, grp, t)[q];
            if (a > 0.0f) lc += log((double)a);
        }
        lp = (float)(log((double)total) + lc);
    }
    r.den_out[seq * 2 + 0] = total;
    r.den_out[seq * 2 + 1] = lp;
}

// ---- posteriors --------------------------------------------------------------------------------------
// gamma_t[pdf] = e[t][pdf] sum_arcs alpha'[t][src] tp beta[t+1][dst] over the rows (pdfs) of the q
// table, every (group, frame) in parallel, written over e[t][pdf]; the frame's sum as partials.
template <int NQ>
__global__ __launch_bounds__(DG_THREADS) void k_dg_post(const DgDev g, const DgRun r) {
    __shared__ float red[DG_WAVES * 64];
    constexpr int R = 64 / NQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane % NQ, sub = lane / NQ, t = blockIdx.y, grp = blockIdx.z;
    const int seq = grp * NQ + q;
    const int T = seq < r.nseq ? r.frames[seq] : 0;
    const bool live = t < T, first = t + 1 == T;
    float ca = 0.f, cb = 0.f;
    if (live) {
        ca = dg_sum(r.w.asum, r, grp, t)[q] * r.leaky;
        cb = r.leaky * (first ? g.as0 : dg_sum(r.w.bsum, r, grp, t + 1)[q]);
    }
    const float *va = dg_alpha(g, r, grp, t);
    const float *vb = t + 1 < r.Tm ? dg_beta(g, r, grp, t + 1) : nullptr;
    float *e = dg_e(g, r, grp, t);
    const int nrg = g.q.nrows / R, W = gridDim.x * DG_WAVES;
    float psum = 0.f;
    for (int rg = blockIdx.x * DG_WAVES + wave; rg < nrg; rg += W) {
        const int row = rg * R + sub;
        const float acc = dg_row_sum<NQ, true>(
            g.q, row, lane,
            [&](bool on, int f1, int f2, float &a, float &b) {
                on = on && live;
                a = on ? va[(size_t)f1 * NQ + q] : 0.0f;
                b = first ? 1.0f : 0.0f;
                if (on && !first) b = vb[(size_t)f2 * NQ + q];
            },
            [&](float a, float b, float tp, float ti) { return (a * tp + ca * ti) * (b + cb); });
        const int pdf = g.q.perm[row];
        if (live && pdf >= 0) {
            const float gv = acc * e[(size_t)pdf * NQ + q];
            e[(size_t)pdf * NQ + q] = gv;
            psum += gv;
        }
    }
    dg_store_partial<NQ>(psum, red, dg_part(r.w.gpart, r, grp, t, r.max_frames));
}

// ---- the objective assembly (k_den_post's product mode, restated for the interleaved rows) ------------
// One block per (group, frame). The frame's posteriors are normalised by their sum and turned into
// -w den in place, the numerator's sparse posteriors are added in place, then 64-pdf tiles go back
// through LDS to the matrix rows: the out-of-range penalty, L2, the frame weight and the grad scale
// before the one rounding to fp16. The frame's out-of-range count and sum x^2 of each sequence are
// left per (sequence, frame): per lane over the tiles in tile order, then the wave butterfly.
template <int NQ>
__global__ __launch_bounds__(DG_THREADS) void k_dg_asm(const DgDev g, const DgRun r, int nwg) {
    __shared__ float red[DG_WAVES * 64];
    __shared__ float tile[64 * (NQ + 1)];
    __shared__ float s_ginv[NQ], s_w[NQ], s_fw[NQ];
    __shared__ int s_ok[NQ], s_live[NQ];
    constexpr int QW = (NQ + DG_WAVES - 1) / DG_WAVES;  // sequences per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x, grp = blockIdx.y, P = g.P;
    const float gsum = dg_resum(dg_part(r.w.gpart, r, grp, t, r.max_frames), nwg, NQ, red);
    if (tid < NQ) {
        const int seq = grp * NQ + tid;
        const int T = seq < r.nseq ? r.frames[seq] : 0;
        float w = r.opts.supervision_weight, fw = 1.0f;
        int ok = 0;
        if (t < T) {
            if (r.seq_w) w *= r.seq_w[seq];
            const double objf = (double)w * ((double)*r.nums[seq].total - (double)r.den_out[seq * 2 + 1]);
            ok = !(isnan(objf) || isinf(objf));
            if (r.frame_w) fw = r.frame_w[(size_t)seq * r.max_frames + t];
            if (r.grad_scale) fw *= *r.grad_scale;
        }
        s_live[tid] = t < T;
        s_ok[tid] = ok;
        s_w[tid] = w;
        s_fw[tid] = fw;
        s_ginv[tid] = gsum > 0.0f ? 1.0f / gsum : 0.0f;
    }
    __syncthreads();
    float *gam = dg_e(g, r, grp, t);
    {  // -w den (DG_THREADS is a multiple of NQ: a thread keeps its q)
        const int q = tid % NQ;
        const float w = s_w[q], ginv = s_ginv[q];
        if (s_live[q])
            for (int idx = tid; idx < P * NQ; idx += DG_THREADS) gam[idx] = -(w * (gam[idx] * ginv));
    }
    __syncthreads();
    for (int q = wave; q < NQ; q += DG_WAVES) {  // + w num on the numerator's pdf set
        if (!s_live[q]) continue;
        const LogFstDev *nf = &r.nums[grp * NQ + q];
        const float *nps = nf->post_sparse + (size_t)t * nf->G;
        const float w = s_w[q];
        for (int k = lane; k < nf->G; k += 64) {
            const int p = nf->grp_pdf[k];
            if (p > 0 && p <= P) gam[(size_t)(p - 1) * NQ + q] = w * nps[k] + gam[(size_t)(p - 1) * NQ + q];
        }
    }
    __syncthreads();
    const h16 *nnet = reinterpret_cast<const h16 *>(r.nnet);
    const float oscale = 2.0f * r.opts.out_of_range_regularize;
    const bool do_oor = r.opts.out_of_range_regularize > 0.0f && (t & 1) == 0;
    const bool do_l2 = r.opts.l2_regularize > 0.0f;
    float oor[QW], sq[QW];
#pragma unroll
    for (int i = 0; i < QW; ++i) oor[i] = sq[i] = 0.f;
    for (int p0 = 0; p0 < P; p0 += 64) {
        for (int idx = tid; idx < 64 * NQ; idx += DG_THREADS) {
            const int q = idx % NQ, pp = idx / NQ;
            tile[pp * (NQ + 1) + q] = p0 + pp < P ? gam[(size_t)(p0 + pp) * NQ + q] : 0.0f;
        }
        __syncthreads();
        const int p = p0 + lane;
#pragma unroll
        for (int i = 0; i < QW; ++i) {
            const int q = wave + i * DG_WAVES;
            if (q >= NQ || !s_live[q] || p >= P) continue;
            const int seq = grp * NQ + q;
            const long long row = r.row0[seq] + (long long)t * r.stride;
            const float x = (float)nnet[row * r.ld + p];
            float d = 0.0f;
            if (do_oor) {  // chain_backward.cu:27-67
                if (x < -30.0f) {
                    d += (-30.0f - x) * oscale;
                    oor[i] += 1.0f;
                } else if (x > 30.0f) {
                    d += (30.0f - x) * oscale;
                    oor[i] += 1.0f;
                }
            }
            d += tile[lane * (NQ + 1) + q];
            if (do_l2) {
                d -= s_w[q] * r.opts.l2_regularize * x;
                sq[i] += x * x;
            }
            r.out_grad[row * r.ldg + p] = s_ok[q] ? (h16)(-(d * s_fw[q])) : (h16)0.0f;  // loss gradient = -deriv
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < QW; ++i) {
        const int q = wave + i * DG_WAVES;
        const float o = wave_sum(oor[i]), s2 = wave_sum(sq[i]);
        if (q < NQ && lane == 0 && s_live[q]) {
            float *fp = r.w.fpart + ((size_t)(grp * NQ + q) * r.max_frames + t) * 2;
            fp[0] = o;
            fp[1] = s2;
        }
    }
}

// stats[8] of every sequence; the per-frame terms in frame order
__global__ void k_dg_stats(const DgRun r) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= r.nseq) return;
    float *st8 = r.stats + (size_t)seq * 8;
    const int T = r.frames[seq];
    if (T <= 0) {  // a sequence without frames adds nothing to kf_chain_result
        for (int i = 0; i < 8; ++i) st8[i] = 0.0f;
        return;
    }
    float w = r.opts.supervision_weight;
    if (r.seq_w) w *= r.seq_w[seq];
    const float num_lp = *r.nums[seq].total, den_lp = r.den_out[seq * 2 + 1];
    const double objf = (double)w * ((double)num_lp - (double)den_lp);
    const bool ok = !(isnan(objf) || isinf(objf));
    const float l2s = w * r.opts.l2_regularize;
    float o = 0.f, l2 = 0.f;
    const float *fp = r.w.fpart + (size_t)seq * r.max_frames * 2;
    for (int t = 0; t < T; ++t) {
        o += fp[2 * t];
        l2 += -0.5f * l2s * fp[2 * t + 1];
    }
    st8[0] = num_lp;
    st8[1] = den_lp;
    st8[2] = ok ? (float)objf : (float)(-10.0 * w * T);  // backward.go:356-363
    st8[3] = r.opts.l2_regularize > 0.0f && ok ? l2 : 0.0f;
    st8[4] = w * (float)T;
    st8[5] = (float)T;
    st8[6] = o;
    st8[7] = ok ? 1.0f : 0.0f;
}

// ===========================================================================
// Host: device tables of a graph, the workspace, launches
// ===========================================================================
static_assert(sizeof(SellRec) == sizeof(uint2), "SellRec is uploaded as the kernels' uint2");

DgTables *make_dg_tables(int S, int P, int A, const int32_t *src, const int32_t *dst, const int32_t *pdf0,
                         const float *tp, const float *init, const char **why) {
    DgHost h;
    if (!den_global_tables(S, P, A, src, dst, pdf0, tp, h, why)) return nullptr;
    auto *t = new DgTables();
    DgDev &d = t->dev;
    d.S = S;
    d.P = P;
    d.A = A;
    d.as0 = 0.f;
    for (int s = 0; s < S; ++s) d.as0 += init[s];
    bool ok = true;
    auto put = [&](DgTabDev &o, const DgTable &ht, bool states) {
        o.nrows = (int)ht.perm.size();
        o.rowptr = dev_upload(ht.rowptr, t->owned);
        o.perm = dev_upload(ht.perm, t->owned);
        o.rec = reinterpret_cast<const uint2 *>(dev_upload(ht.rec, t->owned));
        std::vector<float> ti(ht.rec.size()), ip(ht.perm.size(), 0.0f);
        for (size_t k = 0; k < ti.size(); ++k) {
            float tpk;
            memcpy(&tpk, &ht.rec[k].y, 4);
            ti[k] = tpk * init[ht.isrc[k]];
        }
        for (size_t i = 0; states && i < ip.size(); ++i)
            if (ht.perm[i] >= 0) ip[i] = init[ht.perm[i]];
        o.ti = dev_upload(ti, t->owned);
        o.initp = dev_upload(ip, t->owned);
        ok = ok && o.rowptr && o.perm && o.rec && o.ti && o.initp;
    };
    put(d.f, h.f, true);
    put(d.b, h.b, true);
    put(d.q, h.q, false);
    if (!ok) {
        delete t;
        *why = "hipMalloc failed for den tables";
        return nullptr;
    }
    return t;
}

size_t dg_work_bytes(const DgDev &g, int max_seqs, int max_frames, float *base, DgWork *w) {
    const size_t sl = dg_slots(max_seqs), mf = max_frames, RS = g.f.nrows;
    size_t n = 0;
    auto take = [&](float *&p, size_t words) {
        p = base + n;
        n += (words + 63) / 64 * 64;
    };
    DgWork tmp;
    DgWork &o = w ? *w : tmp;
    take(o.alpha, sl * (mf + 1) * RS);
    take(o.beta, sl * mf * RS);
    take(o.e, sl * mf * g.P);
    take(o.apart, sl * (mf + 1) * DG_MAXWG);
    take(o.bpart, sl * (mf + 1) * DG_MAXWG);
    take(o.gpart, sl * mf * DG_MAXWG);
    take(o.asum, sl * (mf + 1));
    take(o.bsum, sl * (mf + 1));
    take(o.fpart, sl * mf * 2);
    return n * 4;
}

// workgroups of a launch over `nrows` table rows: two passes of a block's 16 waves at least
static int dg_nwg(int nrows, int NQ) {
    const int nrg = nrows / (64 / NQ);
    return std::max(1, std::min(DG_MAXWG, (nrg + 2 * DG_WAVES - 1) / (2 * DG_WAVES)));
}

#define DG_FOR_NQ(NQ_, ...)                                    \
    switch (NQ_) {                                             \
        case 1: { constexpr int Q = 1; __VA_ARGS__; } break;   \
        case 2: { constexpr int Q = 2; __VA_ARGS__; } break;   \
        case 4: { constexpr int Q = 4; __VA_ARGS__; } break;   \
        case 8: { constexpr int Q = 8; __VA_ARGS__; } break;   \
        case 16: { constexpr int Q = 16; __VA_ARGS__; } break; \
        case 32: { constexpr int Q = 32; __VA_ARGS__; } break; \
        default: { constexpr int Q = 64; __VA_ARGS__; } break; \
    }

void launch_dg_recursions(const DgDev &g, const DgRun &r) {
    hipStream_t st = kf_stream();
    if (r.Tm <= 0) {  // no frame anywhere: only the statistics (zeros) follow
        k_dg_lp<<<dim3((r.nseq + 255) / 256), dim3(256), 0, st>>>(g, r);
        return;
    }
    const int nwg = dg_nwg(g.f.nrows, r.NQ);
    k_dg_stage<<<dim3((g.P + 63) / 64, r.Tm, r.ngrp), dim3(256), 0, st>>>(g, r);
    k_dg_row0<<<dim3((g.f.nrows * r.NQ + 255) / 256, r.ngrp), dim3(256), 0, st>>>(g, r);
    const dim3 grid(nwg, r.ngrp), block(DG_THREADS);
    // the two recursions are independent (den_bwd_body); frame by frame, the stream orders them
    for (int t = 0; t < r.Tm; ++t) DG_FOR_NQ(r.NQ, k_dg_rec<Q, 0><<<grid, block, 0, st>>>(g, r, t));
    for (int t = r.Tm - 1; t >= 1; --t) DG_FOR_NQ(r.NQ, k_dg_rec<Q, 1><<<grid, block, 0, st>>>(g, r, t));
    k_dg_sums<<<dim3(r.Tm + 1, r.ngrp), block, 0, st>>>(g, r, nwg);
    k_dg_lp<<<dim3((r.nseq + 255) / 256), dim3(256), 0, st>>>(g, r);
}

void launch_dg_post(const DgDev &g, const DgRun &r) {
    hipStream_t st = kf_stream();
    if (r.Tm > 0) {
        const int nwg = dg_nwg(g.q.nrows, r.NQ);
        const dim3 block(DG_THREADS);
        DG_FOR_NQ(r.NQ, k_dg_post<Q><<<dim3(nwg, r.Tm, r.ngrp), block, 0, st>>>(g, r));
        DG_FOR_NQ(r.NQ, k_dg_asm<Q><<<dim3(r.Tm, r.ngrp), block, 0, st>>>(g, r, nwg));
    }
    k_dg_stats<<<dim3((r.nseq + 255) / 256), dim3(256), 0, st>>>(r);
}
