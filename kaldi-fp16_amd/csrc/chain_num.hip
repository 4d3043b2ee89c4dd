// chain_num.hip — the log-domain numerator of the chain objective: forward-backward of
// one FST per workgroup, all frames in one launch, fixed arc order (the deterministic
// algorithm of chain_det.cu:55-237; posteriors summed per pdf in arc order).
//   k_logfb     any FST, tables in global memory: the chain.h ABI, and batches with an
//               FST too large for the LDS
//   k_num_fb    the product path: the FST in LDS, forwards and backwards in separate
//               workgroups at the same time
//   k_num_post  the posteriors from k_num_fb's stored rows
// with the upload of a batch's FSTs and the host launch entries (chain_num.h).
#include "chain_num.h"

// ===========================================================================
// Log-domain forward-backward (numerator; chain.h ABI)
// ===========================================================================
__global__ __launch_bounds__(256) void k_logfb(const LogFstDev *fsts, const h16 *nnet, long long ld,
                                               int P) {
    const LogFstDev f = fsts[blockIdx.x];
    const int S = f.S, T = f.T, tid = threadIdx.x;
    if (S <= 0 || T < 0) return;
    float total;
    if (f.mode & LF_FB) {
        for (int s = tid; s < S; s += 256) f.alpha[s] = (s == f.start) ? 0.0f : kLogZero;
        __syncthreads();
        for (int t = 0; t < T; ++t) {
            const h16 *xr = nnet + (f.row0 + (long long)t * f.stride) * ld;
            const float *ac = f.alpha + (size_t)t * S;
            float *an = f.alpha + (size_t)(t + 1) * S;
            for (int d = tid; d < S; d += 256) {
                float v = kLogZero;
                for (int k = f.in_ptr[d]; k < f.in_ptr[d + 1]; ++k) {
                    int a = f.in_arc[k];
                    int p = f.arc_pdf[a];
                    if (p <= 0 || p > P) continue;
                    float sa = ac[f.arc_src[a]];
                    if (sa <= kLogZero) continue;
                    v = logadd_dev(v, sa + (float)xr[p - 1] + f.arc_w[a]);
                }
                an[d] = v;
            }
            __syncthreads();
        }
        total = kLogZero;
        for (int i = 0; i < f.nfinal; ++i)
            total = logadd_dev(total, f.alpha[(size_t)T * S + f.fin_state[i]] + f.fin_w[i]);
        if (tid == 0) *f.total = total;
        float *bT = f.beta + (size_t)T * S;
        for (int s = tid; s < S; s += 256) bT[s] = kLogZero;
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < f.nfinal; ++i) bT[f.fin_state[i]] = f.fin_w[i];
        __syncthreads();
    } else {
        total = *f.total;
    }
    for (int t = T - 1; t >= 0; --t) {
        const h16 *xr = nnet + (f.row0 + (long long)t * f.stride) * ld;
        const float *bn = f.beta + (size_t)(t + 1) * S;
        if (f.mode & LF_FB) {
            float *bc = f.beta + (size_t)t * S;
            for (int s = tid; s < S; s += 256) {
                float v = kLogZero;
                for (int a = f.row_ptr[s]; a < f.row_ptr[s + 1]; ++a) {
                    int p = f.arc_pdf[a];
                    if (p <= 0 || p > P) continue;
                    float b = bn[f.arc_dst[a]];
                    if (b <= kLogZero) continue;
                    v = logadd_dev(v, b + (float)xr[p - 1] + f.arc_w[a]);
                }
                bc[s] = v;
            }
        }
        if (f.mode & LF_POST) {
            float *pd = f.post_dense ? f.post_dense + (size_t)t * P : nullptr;
            if (pd) {
                for (int p = tid; p < P; p += 256) pd[p] = 0.0f;
                __syncthreads();
            }
            const float *ac = f.alpha + (size_t)t * S;
            for (int g = tid; g < f.G; g += 256) {
                int p = f.grp_pdf[g];
                float acc = 0.0f;
                if (p > 0 && p <= P) {
                    float xv = (float)xr[p - 1];
                    for (int k = f.grp_ptr[g]; k < f.grp_ptr[g + 1]; ++k) {
                        int a = f.grp_arc[k];
                        float av = ac[f.arc_src[a]];
                        if (av <= kLogZero) continue;
                        float b = bn[f.arc_dst[a]];
                        if (b <= kLogZero) continue;
                        float lp = av + xv + f.arc_w[a] + b - total;
                        if (lp > 0.0f) lp = 0.0f;  // chain.cu:309-311
                        acc += expf(lp);
                    }
                    if (pd) pd[p - 1] = acc;
                }
                if (f.post_sparse) f.post_sparse[(size_t)t * f.G + g] = acc;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Product numerator: the whole FST (arcs pre-gathered per incoming / outgoing /
// pdf-group order) lives in LDS; per frame only the G distinct pdf values of the
// output row are fetched, one frame ahead. Same arithmetic and order as k_logfb.
// ---------------------------------------------------------------------------
#define NUM_THREADS 256
#define NUM_PRE 4  // S, G <= 1024 (larger FSTs use k_logfb)

struct NumLds {  // word offsets into dynamic LDS
    int a0, a1, xg0, xg1, in_ptr, in_src, in_g, in_w, row_ptr, arc_dst, arc_g, arc_w, gpdf, misc, words;
};
__host__ __device__ inline NumLds num_lds_layout(int S, int A, int G, int Ag) {
    (void)Ag;  // the pdf-group arcs are read by k_num_post from global memory
    NumLds L;
    int o = 0;
    L.a0 = o; o += S;
    L.a1 = o; o += S;
    L.xg0 = o; o += G;
    L.xg1 = o; o += G;
    L.in_ptr = o; o += S + 1;
    L.in_src = o; o += A;
    L.in_g = o; o += A;
    L.in_w = o; o += A;
    L.row_ptr = o; o += S + 1;
    L.arc_dst = o; o += A;
    L.arc_g = o; o += A;
    L.arc_w = o; o += A;
    L.gpdf = o; o += G;
    L.misc = o; o += 4;
    L.words = o;
    return L;
}

// Workgroups [0, nseq) run the forwards (alpha rows and the total), [nseq, 2 nseq) the
// backwards at the same time (the backward needs neither alpha nor the total: it stores
// its beta rows); k_num_post then forms the posteriors from the stored rows. (One
// workgroup per sequence running both passes took 2.7 ms alone, 4.6 ms beside the den
// recursion; the split takes 1.8 + 0.7 ms and costs the recursion ~0.25 ms less.)
__global__ __launch_bounds__(NUM_THREADS) void k_num_fb(const LogFstDev *fsts, const h16 *nnet,
                                                        long long ld, int P, int nseq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const bool do_fwd = (int)blockIdx.x < nseq;
    const LogFstDev f = fsts[(int)blockIdx.x % nseq];
    const int S = f.S, A = f.A, G = f.G, T = f.T, tid = threadIdx.x;
    const int Ag = f.G > 0 ? f.grp_ptr[f.G] : 0;
    const NumLds L = num_lds_layout(S, A, G, Ag);
    float *W = reinterpret_cast<float *>(smem);
    int *I = reinterpret_cast<int *>(smem);
    // stage the FST; arcs whose pdf is outside [1, P] get group -1 (skipped)
    for (int i = tid; i <= S; i += NUM_THREADS) {
        I[L.in_ptr + i] = f.in_ptr[i];
        I[L.row_ptr + i] = f.row_ptr[i];
    }
    for (int q = tid; q < G; q += NUM_THREADS) I[L.gpdf + q] = f.grp_pdf[q];
    for (int k = tid; k < A; k += NUM_THREADS) {
        int g0 = f.in_g[k], g1 = f.arc_g[k];
        int p0 = g0 >= 0 ? f.grp_pdf[g0] : 0, p1 = g1 >= 0 ? f.grp_pdf[g1] : 0;
        I[L.in_src + k] = f.in_src[k];
        I[L.in_g + k] = (p0 > 0 && p0 <= P) ? g0 : -1;
        W[L.in_w + k] = f.in_w[k];
        I[L.arc_dst + k] = f.arc_dst[k];
        I[L.arc_g + k] = (p1 > 0 && p1 <= P) ? g1 : -1;
        W[L.arc_w + k] = f.arc_w[k];
    }
    float *cur = W + L.a0, *nxt = W + L.a1;
    if (do_fwd)
        for (int s = tid; s < S; s += NUM_THREADS) {
            float v = (s == f.start) ? 0.0f : kLogZero;
            cur[s] = v;
            f.alpha[s] = v;
        }
    __syncthreads();
    auto row_of = [&](int t) { return nnet + (f.row0 + (long long)t * f.stride) * ld; };
    float pre[NUM_PRE];
    auto fetch_x = [&](int t) {
        const h16 *xr = row_of(t);
#pragma unroll
        for (int i = 0; i < NUM_PRE; ++i) {  // unconditional (clamped) loads, then select
            int q = tid + i * NUM_THREADS;
            int p = q < G ? I[L.gpdf + q] : 0;
            float v = (float)xr[min(max(p, 1), P) - 1];
            pre[i] = (p > 0 && p <= P) ? v : 0.0f;
        }
    };
    auto store_x = [&](float *xg) {
#pragma unroll
        for (int i = 0; i < NUM_PRE; ++i) {
            int q = tid + i * NUM_THREADS;
            if (q < G) xg[q] = pre[i];
        }
    };
    // ---- forward
    if (do_fwd) {
    if (T > 0) {
        fetch_x(0);
        store_x(W + L.xg0);
        if (T > 1) fetch_x(1);
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const float *xg = W + ((t & 1) ? L.xg1 : L.xg0);
        float *an = f.alpha + (size_t)(t + 1) * S;
        for (int d = tid; d < S; d += NUM_THREADS) {
            float v = kLogZero;
            for (int k = I[L.in_ptr + d]; k < I[L.in_ptr + d + 1]; ++k) {
                int g = I[L.in_g + k];
                if (g < 0) continue;
                float sa = cur[I[L.in_src + k]];
                if (sa <= kLogZero) continue;
                v = logadd_dev(v, sa + xg[g] + W[L.in_w + k]);
            }
            nxt[d] = v;
            an[d] = v;
        }
        if (t + 1 < T) {
            store_x(W + ((t & 1) ? L.xg0 : L.xg1));
            if (t + 2 < T) fetch_x(t + 2);
        }
        __syncthreads();
        float *tmp = cur;
        cur = nxt;
        nxt = tmp;
    }
    // total over the finals, in order (chain.cu:213-240)
    if (tid == 0) {
        float tot = kLogZero;
        for (int i = 0; i < f.nfinal; ++i) tot = logadd_dev(tot, cur[f.fin_state[i]] + f.fin_w[i]);
        W[L.misc] = tot;
        *f.total = tot;
    }
        return;
    }  // forward
    // ---- backward: beta rows into f.beta (rows 0 .. T)
    float *bn = W + L.a0, *bc = W + L.a1;  // beta[t+1], beta[t]
    __syncthreads();
    for (int s = tid; s < S; s += NUM_THREADS) bn[s] = kLogZero;
    if (T > 0) {
        fetch_x(T - 1);
        store_x(W + L.xg0);
        if (T > 1) fetch_x(T - 2);
    }
    __syncthreads();
    if (tid == 0)
        for (int i = 0; i < f.nfinal; ++i) bn[f.fin_state[i]] = f.fin_w[i];
    __syncthreads();
    for (int s = tid; s < S; s += NUM_THREADS) f.beta[(size_t)T * S + s] = bn[s];
    for (int t = T - 1, it = 0; t >= 0; --t, ++it) {
        const float *xg = W + ((it & 1) ? L.xg1 : L.xg0);
        for (int s = tid; s < S; s += NUM_THREADS) {
            float v = kLogZero;
            for (int k = I[L.row_ptr + s]; k < I[L.row_ptr + s + 1]; ++k) {
                int g = I[L.arc_g + k];
                if (g < 0) continue;
                float b = bn[I[L.arc_dst + k]];
                if (b <= kLogZero) continue;
                v = logadd_dev(v, b + xg[g] + W[L.arc_w + k]);
            }
            bc[s] = v;
            f.beta[(size_t)t * S + s] = v;
        }
        if (t > 0) {
            store_x(W + ((it & 1) ? L.xg0 : L.xg1));
            if (t > 1) fetch_x(t - 2);
        }
        __syncthreads();
        float *tmp = bn;
        bn = bc;
        bc = tmp;
    }
}

// posteriors of the numerator (after k_num_fb): one workgroup per (sequence,
// NUM_POST_FR frames) from the stored alpha[t], beta[t+1] and the total — the arithmetic
// and order of k_num_fb's fused posterior loop
#define NUM_POST_FR 8
__global__ __launch_bounds__(NUM_THREADS) void k_num_post(const LogFstDev *fsts, const h16 *nnet, long long ld,
                                                          int P, int nfb) {
    const LogFstDev f = fsts[blockIdx.x / nfb];
    const int t0 = (blockIdx.x % nfb) * NUM_POST_FR;
    const float total = *f.total;
    for (int t = t0; t < min(f.T, t0 + NUM_POST_FR); ++t) {
    const float *ar = f.alpha + (size_t)t * f.S, *bn = f.beta + (size_t)(t + 1) * f.S;
    const h16 *xr = nnet + (f.row0 + (long long)t * f.stride) * ld;
    float *ps = f.post_sparse + (size_t)t * f.G;
    for (int q = threadIdx.x; q < f.G; q += NUM_THREADS) {
        const int p = f.grp_pdf[q];
        float acc = 0.0f;
        if (p > 0 && p <= P) {
            const float xv = (float)xr[p - 1];
            for (int k = f.grp_ptr[q]; k < f.grp_ptr[q + 1]; ++k) {
                float av = ar[f.gsrc[k]];
                if (av <= kLogZero) continue;
                float b = bn[f.gdst[k]];
                if (b <= kLogZero) continue;
                float lp = av + xv + f.gw[k] + b - total;
                if (lp > 0.0f) lp = 0.0f;  // chain.cu:309-311
                acc += expf(lp);
            }
        }
        ps[q] = acc;
    }
    }
}

// ===========================================================================
// Host: upload and launches
// ===========================================================================
void num_descs(const std::vector<NumHost> &hs, const std::vector<std::vector<size_t>> &offs,
               const int32_t *d, NumDevice *nd) {
    nd->desc.clear();
    nd->G.clear();
    nd->Ag.clear();
    for (size_t i = 0; i < hs.size(); ++i) {
        const auto &o = offs[i];
        LogFstDev f{};
        f.row_ptr = d + o[0];
        f.in_ptr = d + o[1];
        f.in_arc = d + o[2];
        f.arc_src = d + o[3];
        f.arc_dst = d + o[4];
        f.arc_pdf = d + o[5];
        f.arc_w = reinterpret_cast<const float *>(d + o[6]);
        f.grp_ptr = d + o[7];
        f.grp_pdf = d + o[8];
        f.grp_arc = d + o[9];
        f.fin_state = d + o[10];
        f.fin_w = reinterpret_cast<const float *>(d + o[11]);
        f.in_src = d + o[12];
        f.in_g = d + o[13];
        f.arc_g = d + o[14];
        f.gsrc = d + o[15];
        f.gdst = d + o[16];
        f.in_w = reinterpret_cast<const float *>(d + o[17]);
        f.gw = reinterpret_cast<const float *>(d + o[18]);
        f.S = hs[i].S;
        f.A = hs[i].A;
        f.G = (int)hs[i].grp_pdf.size();
        f.nfinal = hs[i].nfinal;
        f.start = hs[i].start;
        nd->desc.push_back(f);
        nd->G.push_back(f.G);
        nd->Ag.push_back((int)hs[i].grp_arc.size());
    }
}

NumDevice *upload_nums(std::vector<NumHost> &hs, const char **why) {
    std::vector<int32_t> blob;
    std::vector<std::vector<size_t>> offs;
    pack_nums(hs, blob, offs);
    auto *nd = new NumDevice();
    int32_t *d = dev_upload(blob, nd->owned);
    if (!d) {
        delete nd;
        *why = "hipMalloc failed for numerator FSTs";
        return nullptr;
    }
    num_descs(hs, offs, d, nd);
    return nd;
}

bool fetch_fst(const ChainFstGPU *fst, NumHost &h, const char **why) {
    if (!fst || fst->num_states <= 0 || fst->num_arcs < 0 || fst->num_final < 0) {
        *why = "invalid ChainFstGPU";
        return false;
    }
    h.S = fst->num_states;
    h.A = fst->num_arcs;
    h.nfinal = fst->num_final;
    h.start = fst->start_state;
    h.row_ptr.resize(h.S + 1);
    h.arc_dst.resize(h.A);
    h.arc_pdf.resize(h.A);
    h.arc_w.resize(h.A);
    h.fin_state.resize(h.nfinal);
    h.fin_w.resize(h.nfinal);
    hipStreamSynchronize(kf_stream());
    bool ok = hipMemcpy(h.row_ptr.data(), fst->row_ptr, (h.S + 1) * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (h.A) {
        ok = ok && hipMemcpy(h.arc_dst.data(), fst->col_idx, h.A * 4, hipMemcpyDeviceToHost) == hipSuccess;
        ok = ok && hipMemcpy(h.arc_pdf.data(), fst->labels, h.A * 4, hipMemcpyDeviceToHost) == hipSuccess;
        ok = ok && hipMemcpy(h.arc_w.data(), fst->weights, h.A * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (h.nfinal) {
        ok = ok && hipMemcpy(h.fin_state.data(), fst->final_states, h.nfinal * 4, hipMemcpyDeviceToHost) == hipSuccess;
        ok = ok && hipMemcpy(h.fin_w.data(), fst->final_weights, h.nfinal * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) {
        *why = "device->host copy of the FST failed";
        return false;
    }
    return prepare_num(h, why);
}

bool run_logfb(std::vector<LogFstDev> &fsts, const void *nnet16, long long ld, int P,
               std::vector<float> &totals, const char **why) {
    kf_take_pending(__func__);
    DevBuf d, tot;
    size_t n = fsts.size();
    if (!tot.alloc(n * sizeof(float)) || !d.alloc(n * sizeof(LogFstDev))) {
        *why = "hipMalloc failed";
        return false;
    }
    hipStream_t st = kf_stream();
    for (size_t i = 0; i < n; ++i)
        if (!(fsts[i].mode & LF_FB)) {
            hipMemcpyAsync((float *)tot.p + i, &totals[i], 4, hipMemcpyHostToDevice, st);
        }
    for (size_t i = 0; i < n; ++i) fsts[i].total = (float *)tot.p + i;
    hipMemcpyAsync(d.p, fsts.data(), n * sizeof(LogFstDev), hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(k_logfb, dim3(n), dim3(256), 0, st, (const LogFstDev *)d.p,
                       (const h16 *)nnet16, ld, P);
    totals.resize(n);
    hipMemcpyAsync(totals.data(), tot.p, n * 4, hipMemcpyDeviceToHost, st);
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess || hipGetLastError() != hipSuccess) {
        *why = hipGetErrorString(e);
        return false;
    }
    return true;
}

size_t num_batch_lds(const std::vector<LogFstDev> &desc, const std::vector<int> &Ag, int nseq) {
    size_t lds = 0;
    bool fits = true;
    for (int i = 0; i < nseq; ++i) {
        const LogFstDev &f = desc[i];
        lds = std::max(lds, (size_t)num_lds_layout(f.S, f.A, f.G, Ag[i]).words * 4);
        fits = fits && f.S <= NUM_PRE * NUM_THREADS && f.G <= NUM_PRE * NUM_THREADS;
    }
    return (fits && lds <= 64 * 1024) ? lds : 0;
}

void launch_num_batch(const LogFstDev *fsts, const h16 *nnet, long long ld, int P, int nseq, int maxT,
                      size_t num_lds, hipStream_t st) {
    if (num_lds) {
        // forwards and backwards at the same time, then the posteriors (the numerator
        // shares CUs with the den recursion: the shorter, the less it costs it)
        hipLaunchKernelGGL(k_num_fb, dim3(2 * nseq), dim3(NUM_THREADS), num_lds, st, fsts, nnet, ld, P, nseq);
        const int nfb = (maxT + NUM_POST_FR - 1) / NUM_POST_FR;
        if (maxT > 0)
            hipLaunchKernelGGL(k_num_post, dim3(nseq * nfb), dim3(NUM_THREADS), 0, st, fsts, nnet, ld, P, nfb);
    } else {
        hipLaunchKernelGGL(k_logfb, dim3(nseq), dim3(256), 0, st, fsts, nnet, ld, P);
    }
}
