// chain_abi.hip — the reference C-ABIs of the chain objective, served by the numerator
// and denominator units' kernels (chain_num.hip, chain_den.hip):
//   chain.h               log-domain forward-backward, posteriors, loss (k_logfb)
//   chain_backward_api.h  element-wise objective pieces (the small kernels below)
//   chain_den.h           probability-space denominator on uploaded graphs
// and their two thread-local error slots.
#include "chain_denom.h"
#include "chain_num.h"
#include "../../include/chain_backward_api.h"
#include "../../include/chain_den.h"
#include "../../include/kf_ops.h"

#include <map>
#include <mutex>

KF_DECLARE_ERR(chain)
KF_DECLARE_ERR(den)

extern "C" const char *chain_last_error(void) { return chain_err_.get(); }
extern "C" void chain_clear_error(void) { chain_err_.clear(); }
extern "C" const char *den_last_error(void) { return den_err_.get(); }
extern "C" void den_clear_error(void) { den_err_.clear(); }

// ===========================================================================
// chain.h ABI
// ===========================================================================
extern "C" size_t chain_workspace_bytes(int T, int num_states) {
    return 2 * (size_t)(T + 1) * num_states * sizeof(float);
}

static int fb_common(const void *nnet, const ChainFstGPU *fst, int T, int P, float *alpha,
                     float *beta, float *total, int mode, const float *post_in_total,
                     float *post) {
    const char *why = nullptr;
    if (!nnet || !alpha || !beta || T < 0 || P <= 0) {
        chain_set_error("chain_forward_backward: invalid arguments");
        return -1;
    }
    NumHost h;
    if (!fetch_fst(fst, h, &why)) {
        chain_set_error("chain_forward_backward: %s", why);
        return -1;
    }
    std::vector<NumHost> hs{h};
    NumDevice *nd = upload_nums(hs, &why);
    if (!nd) {
        chain_set_error("chain_forward_backward: %s", why);
        return -1;
    }
    std::vector<LogFstDev> fs{nd->desc[0]};
    LogFstDev &f = fs[0];
    // the caller's own arrays are authoritative for arcs and finals
    f.arc_dst = fst->col_idx;
    f.arc_pdf = fst->labels;
    f.arc_w = fst->weights;
    f.fin_state = fst->final_states;
    f.fin_w = fst->final_weights;
    f.T = T;
    f.mode = mode;
    f.stride = 1;
    f.row0 = 0;
    f.alpha = alpha;
    f.beta = beta;
    f.post_dense = post;
    std::vector<float> tot{post_in_total ? *post_in_total : 0.0f};
    bool ok = run_logfb(fs, nnet, P, P, tot, &why);
    delete nd;
    if (!ok) {
        chain_set_error("chain_forward_backward: %s", why);
        return -1;
    }
    if (total) *total = tot[0];
    return 0;
}

extern "C" int chain_forward_backward(const void *nnet_output, const ChainFstGPU *fst, int T,
                                      int num_pdfs, float *alpha, float *beta,
                                      float *total_logprob) {
    return fb_common(nnet_output, fst, T, num_pdfs, alpha, beta, total_logprob, LF_FB, nullptr,
                     nullptr);
}
extern "C" int chain_forward_backward_det(const void *nnet_output, const ChainFstGPU *fst, int T,
                                          int num_pdfs, float *alpha, float *beta,
                                          float *total_logprob) {
    return chain_forward_backward(nnet_output, fst, T, num_pdfs, alpha, beta, total_logprob);
}
extern "C" int chain_compute_posteriors(const void *nnet_output, const ChainFstGPU *fst, int T,
                                        int num_pdfs, const float *alpha, const float *beta,
                                        float total_logprob, float *posteriors) {
    if (!posteriors) {
        chain_set_error("chain_compute_posteriors: posteriors is NULL");
        return -1;
    }
    return fb_common(nnet_output, fst, T, num_pdfs, const_cast<float *>(alpha),
                     const_cast<float *>(beta), nullptr, LF_POST, &total_logprob, posteriors);
}
extern "C" int chain_compute_posteriors_det(const void *nnet_output, const ChainFstGPU *fst,
                                            int T, int num_pdfs, const float *alpha,
                                            const float *beta, float total_logprob,
                                            float *posteriors) {
    return chain_compute_posteriors(nnet_output, fst, T, num_pdfs, alpha, beta, total_logprob,
                                    posteriors);
}

__global__ void k_chain_gradient(h16 *g, const float *num, const float *den, long long n, float w) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = (den[i] - num[i]) * w;  // chain.cu:330-352
    g[i] = (h16)fmaxf(-30.0f, fminf(30.0f, v));
}

extern "C" int chain_compute_loss(const void *nnet_output, const ChainFstGPU *num_fst,
                                  const ChainFstGPU *den_fst, int T, int num_pdfs,
                                  void *grad_output, ChainLossResult *result) {
    const char *why = nullptr;
    if (!nnet_output || !result || T < 0 || num_pdfs <= 0) {
        chain_set_error("chain_compute_loss: invalid arguments");
        return -1;
    }
    std::vector<NumHost> hs(2);
    if (!fetch_fst(num_fst, hs[0], &why) || !fetch_fst(den_fst, hs[1], &why)) {
        chain_set_error("chain_compute_loss: %s", why);
        return -1;
    }
    NumDevice *nd = upload_nums(hs, &why);
    if (!nd) {
        chain_set_error("chain_compute_loss: %s", why);
        return -1;
    }
    const size_t TP = (size_t)T * num_pdfs;
    DevBuf ws, post;
    size_t wsn = 2 * (size_t)(T + 1) * (hs[0].S + hs[1].S);
    if (!ws.alloc(wsn * 4) || !post.alloc(2 * TP * 4)) {
        delete nd;
        chain_set_error("chain_compute_loss: hipMalloc failed");
        return -1;
    }
    std::vector<LogFstDev> fs = nd->desc;
    float *w = (float *)ws.p;
    for (int i = 0; i < 2; ++i) {
        fs[i].T = T;
        fs[i].mode = LF_FB | (grad_output ? LF_POST : 0);
        fs[i].stride = 1;
        fs[i].row0 = 0;
        fs[i].alpha = w;
        w += (size_t)(T + 1) * hs[i].S;
        fs[i].beta = w;
        w += (size_t)(T + 1) * hs[i].S;
        fs[i].post_dense = grad_output ? (float *)post.p + i * TP : nullptr;
    }
    std::vector<float> tot(2, 0.0f);
    bool ok = run_logfb(fs, nnet_output, num_pdfs, num_pdfs, tot, &why);
    delete nd;
    if (!ok) {
        chain_set_error("chain_compute_loss: %s", why);
        return -1;
    }
    result->num_logprob = tot[0];
    result->den_logprob = tot[1];
    result->loss = -(tot[0] - tot[1]);
    if (grad_output && TP) {
        hipLaunchKernelGGL(k_chain_gradient, dim3(kf_blocks(TP, 256)), dim3(256), 0, kf_stream(),
                           (h16 *)grad_output, (const float *)post.p, (const float *)post.p + TP,
                           (long long)TP, 1.0f);
        if (hipStreamSynchronize(kf_stream()) != hipSuccess) {
            chain_set_error("chain_compute_loss: gradient kernel failed");
            return -1;
        }
    }
    return 0;
}

__global__ void k_f32_to_f16(const float *in, h16 *out, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (h16)in[i];
}

static float num_fb_fp32(const int *row_ptr, const int *col_idx, const float *weights,
                         const int *pdf_ids, const int *final_states, const float *final_weights,
                         int S, int A, int F, const float *nnet, float *num_post, int T, int P,
                         void *stream) {
    if (!nnet || !num_post || T < 0 || P <= 0) {
        chain_set_error("chain_num_forward_backward: invalid arguments");
        return -1e30f;
    }
    hipStream_t saved = kf_stream();
    if (stream) kf_set_stream(stream);
    ChainFstGPU fst{(int32_t *)row_ptr, (int32_t *)col_idx, (int32_t *)pdf_ids, (float *)weights,
                    (int32_t *)final_states, (float *)final_weights, S, A, F, 0};
    const size_t TP = (size_t)T * P;
    DevBuf x16, ws;
    float result = -1e30f;
    if (x16.alloc(TP * 2) && ws.alloc(chain_workspace_bytes(T, S))) {
        hipLaunchKernelGGL(k_f32_to_f16, dim3(kf_blocks(TP, 256)), dim3(256), 0, kf_stream(),
                           nnet, (h16 *)x16.p, (long long)TP);
        float *a = (float *)ws.p, *b = a + (size_t)(T + 1) * S;
        float tot = 0.f;
        if (fb_common(x16.p, &fst, T, P, a, b, &tot, LF_FB | LF_POST, nullptr, num_post) == 0)
            result = tot;
    } else {
        chain_set_error("chain_num_forward_backward: hipMalloc failed");
    }
    if (stream) kf_set_stream((void *)saved);
    return result;
}

extern "C" float chain_num_forward_backward(const int *fst_row_ptr, const int *fst_col_idx,
                                            const float *fst_weights, const int *fst_pdf_ids,
                                            const int *fst_final_states,
                                            const float *fst_final_weights, int num_states,
                                            int num_arcs, int num_final, const float *nnet_output,
                                            float *num_post, int T, int num_pdfs, void *stream) {
    return num_fb_fp32(fst_row_ptr, fst_col_idx, fst_weights, fst_pdf_ids, fst_final_states,
                       fst_final_weights, num_states, num_arcs, num_final, nnet_output, num_post,
                       T, num_pdfs, stream);
}
extern "C" float chain_num_forward_backward_det(
    const int *fst_row_ptr, const int *fst_col_idx, const float *fst_weights,
    const int *fst_pdf_ids, const int *fst_final_states, const float *fst_final_weights,
    int num_states, int num_arcs, int num_final, const float *nnet_output, float *num_post, int T,
    int num_pdfs, void *stream) {
    return chain_num_forward_backward(fst_row_ptr, fst_col_idx, fst_weights, fst_pdf_ids, fst_final_states,
                                      fst_final_weights, num_states, num_arcs, num_final, nnet_output,
                                      num_post, T, num_pdfs, stream);
}

// ===========================================================================
// chain_backward_api.h ABI (element-wise objective pieces)
// ===========================================================================
__global__ void k_combine16(const float *num, const float *den, float w, h16 *g, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = (h16)(w * (num[i] - den[i]));
}
__global__ void k_add_post(const float *num, const float *den, float *g, float w, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] += w * (num[i] - den[i]);
}
__global__ void k_penalize(const float *x, float *g, float limit, float scale, int T, int P,
                           int *count) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int c = 0;
    if (i < (long long)T * P && ((i / P) % 2) == 0) {
        float v = x[i];
        if (v < -limit) {
            g[i] += (-limit - v) * scale;
            c = 1;
        } else if (v > limit) {
            g[i] += (limit - v) * scale;
            c = 1;
        }
    }
    float cf = wave_sum((float)c);
    if ((threadIdx.x & 63) == 0 && cf > 0.0f) atomicAdd(count, (int)cf);
}
__global__ void k_l2(const float *x, float *g, float s, long long n, double *acc) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double q = 0.0;
    if (i < n) {
        float v = x[i];
        g[i] -= s * v;
        q = (double)v * v;
    }
    q = wave_sum_d(q);
    if ((threadIdx.x & 63) == 0) atomicAdd(acc, q);
}

extern "C" int chain_combine_gradient(const float *num_post, const float *den_post, float weight,
                                      int T, int num_pdfs, void *grad_output) {
    kf_take_pending(__func__);
    long long n = (long long)T * num_pdfs;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_combine16, dim3(kf_blocks(n, 256)), dim3(256), 0, kf_stream(), num_post,
                       den_post, weight, (h16 *)grad_output, n);
    if (hipGetLastError() != hipSuccess) {
        chain_set_error("chain_combine_gradient: launch failed");
        return -1;
    }
    return 0;
}
extern "C" int chain_add_posterior_gradient(const float *num_post, const float *den_post,
                                            float *grad, float weight, int total_elements) {
    kf_take_pending(__func__);
    if (total_elements <= 0) return 0;
    hipLaunchKernelGGL(k_add_post, dim3(kf_blocks(total_elements, 256)), dim3(256), 0, kf_stream(),
                       num_post, den_post, grad, weight, (long long)total_elements);
    if (hipGetLastError() != hipSuccess) {
        chain_set_error("chain_add_posterior_gradient: launch failed");
        return -1;
    }
    return 0;
}
extern "C" int chain_penalize_out_of_range(const float *nnet_output, float *grad_output,
                                           float limit, float scale, int T, int num_pdfs) {
    long long n = (long long)T * num_pdfs;
    if (n <= 0) return 0;
    DevBuf cnt;
    if (!cnt.alloc(4)) return 0;
    hipStream_t st = kf_stream();
    hipMemsetAsync(cnt.p, 0, 4, st);
    hipLaunchKernelGGL(k_penalize, dim3(kf_blocks(n, 256)), dim3(256), 0, st, nnet_output,
                       grad_output, limit, scale, T, num_pdfs, (int *)cnt.p);
    int h = 0;
    hipMemcpyAsync(&h, cnt.p, 4, hipMemcpyDeviceToHost, st);
    hipStreamSynchronize(st);
    return h;
}
extern "C" float chain_l2_regularize(const float *nnet_output, float *grad_output, float l2_scale,
                                     int total_elements) {
    if (total_elements <= 0) return 0.0f;
    DevBuf acc;
    if (!acc.alloc(8)) return 0.0f;
    hipStream_t st = kf_stream();
    hipMemsetAsync(acc.p, 0, 8, st);
    hipLaunchKernelGGL(k_l2, dim3(kf_blocks(total_elements, 256)), dim3(256), 0, st, nnet_output,
                       grad_output, l2_scale, (long long)total_elements, (double *)acc.p);
    double h = 0.0;
    hipMemcpyAsync(&h, acc.p, 8, hipMemcpyDeviceToHost, st);
    hipStreamSynchronize(st);
    return (float)(-0.5 * l2_scale * h);
}
extern "C" int chain_grad_fp32_to_fp16(const float *grad_fp32, void *grad_fp16,
                                       int total_elements) {
    if (total_elements <= 0) return 0;
    hipLaunchKernelGGL(k_f32_to_f16, dim3(kf_blocks(total_elements, 256)), dim3(256), 0,
                       kf_stream(), grad_fp32, (h16 *)grad_fp16, (long long)total_elements);
    return 0;
}

// ===========================================================================
// chain_den.h ABI
// ===========================================================================
static std::mutex g_den_mu;
static std::map<const void *, DenTables *> g_den_tables;  // keyed by DenFstGPU::src_states

extern "C" int den_fst_upload(DenFstGPU *fst, const int32_t *src, const int32_t *dst,
                              const int32_t *pdf, const float *trans_probs, int num_trans,
                              int num_states, int num_pdfs) {
    const char *why = nullptr;
    if (!fst || !src || !dst || !pdf || !trans_probs) {
        den_set_error("den_fst_upload: NULL argument");
        return -1;
    }
    DenTables *t = make_den_tables(num_states, num_pdfs, num_trans, src, dst, pdf, trans_probs, &why);
    if (!t) {
        den_set_error("den_fst_upload: %s", why);
        return -1;
    }
    std::vector<int32_t> vs(src, src + num_trans), vd(dst, dst + num_trans), vp(pdf, pdf + num_trans);
    std::vector<float> vt(trans_probs, trans_probs + num_trans);
    std::vector<void *> owned;
    fst->src_states = dev_upload(vs, owned);
    fst->dst_states = dev_upload(vd, owned);
    fst->pdf_ids = dev_upload(vp, owned);
    fst->transition_probs = dev_upload(vt, owned);
    if (!fst->src_states || !fst->dst_states || !fst->pdf_ids || !fst->transition_probs) {
        for (void *p : owned) hipFree(p);
        delete t;
        den_set_error("den_fst_upload: hipMalloc failed");
        return -1;
    }
    fst->num_transitions = num_trans;
    fst->num_states = num_states;
    fst->num_pdfs = num_pdfs;
    std::lock_guard<std::mutex> lk(g_den_mu);
    g_den_tables[fst->src_states] = t;
    return 0;
}

extern "C" void den_fst_free(DenFstGPU *fst) {
    if (!fst) return;
    {
        std::lock_guard<std::mutex> lk(g_den_mu);
        auto it = g_den_tables.find(fst->src_states);
        if (it != g_den_tables.end()) {
            delete it->second;
            g_den_tables.erase(it);
        }
    }
    hipFree(fst->src_states);
    hipFree(fst->dst_states);
    hipFree(fst->pdf_ids);
    hipFree(fst->transition_probs);
    fst->src_states = fst->dst_states = fst->pdf_ids = nullptr;
    fst->transition_probs = nullptr;
}

static float den_abi(const DenFstGPU *fst, const float *h_nnet, const float *h_init, int T,
                     float leaky, float *h_post) {
    kf_take_pending(__func__);
    DenTables *t = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_den_mu);
        auto it = fst ? g_den_tables.find(fst->src_states) : g_den_tables.end();
        if (it != g_den_tables.end()) t = it->second;
    }
    if (!t) {
        den_set_error("den_forward: FST was not uploaded with den_fst_upload");
        return -1e30f;
    }
    if (!h_nnet || !h_init || T < 0) {
        den_set_error("den_forward: invalid arguments");
        return -1e30f;
    }
    const int S = t->dev.S, P = t->dev.P;
    const size_t TP = (size_t)T * P;
    DevBuf x, init, as, bs, ast, bst, stats, post, row0, frames, dout;
    const size_t rs = (size_t)t->dev.f.nsl * 64;  // slice-ordered rows
    if (!x.alloc(TP * 4) || !init.alloc(S * 4) || !as.alloc((size_t)(T + 1) * rs * 4) ||
        (h_post && !bs.alloc((size_t)(T + 1) * rs * 4)) ||
        !ast.alloc((T + 1) * 4) || !bst.alloc((T + 1) * 4) || !stats.alloc(32) || !row0.alloc(8) || !frames.alloc(4) ||
        !dout.alloc(8) ||
        (h_post && !post.alloc(TP * 4))) {
        den_set_error("den_forward: hipMalloc failed");
        return -1e30f;
    }
    hipStream_t st = kf_stream();
    long long r0 = 0;
    hipMemcpyAsync(x.p, h_nnet, TP * 4, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(init.p, h_init, S * 4, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(row0.p, &r0, 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(frames.p, &T, 4, hipMemcpyHostToDevice, st);
    DenDev g = t->dev;
    g.init = (const float *)init.p;
    den_tables_set_init(g, g.init, st);
    DenRun r{};
    r.nnet = x.p;
    r.ld = P;
    r.row0 = (const long long *)row0.p;
    r.frames = (const int *)frames.p;
    r.stride = 1;
    r.max_frames = T;
    r.leaky = leaky;
    r.backward = h_post != nullptr;
    r.alpha_store = (float *)as.p;
    r.beta_store = (float *)bs.p;
    r.asum_store = (float *)ast.p;
    r.bsum_store = (float *)bst.p;
    r.stats = (float *)stats.p;
    r.post_dense = (float *)post.p;
    r.den_out = (float *)dout.p;
    DenX X{}, XB{};
    DenXBuf xbuf, xbuf2;
    const int G = h_post ? den_pick_G(2) : den_pick_G(1);
    if (!xbuf.make(g, g.f, 1, 1, G, X) || (h_post && !xbuf2.make(g, g.b, 1, 1, G, XB))) {
        den_set_error("den_forward: hipMalloc failed");
        return -1e30f;
    }
    if (h_post) {
        launch_den_fb(g, r, X, xbuf, XB, xbuf2, true);
        launch_den_post(g, r, X, true, DEN_ABI);
    } else {
        launch_den_fwd(g, r, X, xbuf, true);
    }
    float st8[8] = {0};
    hipMemcpyAsync(st8, stats.p, 32, hipMemcpyDeviceToHost, st);
    if (h_post) hipMemcpyAsync(h_post, post.p, TP * 4, hipMemcpyDeviceToHost, st);
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess || hipGetLastError() != hipSuccess) {
        den_set_error("den_forward_backward: %s", hipGetErrorString(e));
        return -1e30f;
    }
    if (xbuf.take_timeouts(st) + (h_post ? xbuf2.take_timeouts(st) : 0u)) {
        den_set_error("den_forward_backward: cross-workgroup exchange timed out");
        return -1e30f;
    }
    return st8[1];
}

extern "C" float den_forward(const DenFstGPU *fst, const float *nnet_output,
                             const float *initial_probs, int T, float leaky_hmm_coeff) {
    return den_abi(fst, nnet_output, initial_probs, T, leaky_hmm_coeff, nullptr);
}
extern "C" float den_forward_backward(const DenFstGPU *fst, const float *nnet_output,
                                      const float *initial_probs, int T, float leaky_hmm_coeff,
                                      float *grad_output) {
    if (!grad_output) {
        den_set_error("den_forward_backward: grad_output is NULL");
        return -1e30f;
    }
    return den_abi(fst, nnet_output, initial_probs, T, leaky_hmm_coeff, grad_output);
}
