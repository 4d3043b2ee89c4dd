// chain.hip — kf_chain.h, the batched, device-resident product interface of the chain
// LF-MMI objective on MI355X (gfx950): denominator graphs, numerator batches and their
// refill, and kf_chain_compute, which writes the fp16 gradient rows straight into the
// network's output-gradient matrix. Workgroup-resident kernels replace the reference's
// per-frame launch storms (chain.cu launches T kernels per pass with CAS
// atomics; chain_den.cu ~10 launches + 3 blocking D2H copies per frame). Where the parts
// live:
//   chain_tables.cpp  host-side table builders and graph validation, no HIP
//   chain_num.hip     numerator: k_num_fb + k_num_post (FST in LDS), k_logfb (any FST, ABI)
//   chain_den.hip     denominator: k_den_fwd, k_den_fb, k_den_post, the exchange
//   chain_xent.hip    the xent output's derivative and objective: k_chain_xent (kf_chain_xent)
//   chain_abi.hip     the reference ABIs chain.h, chain_backward_api.h, chain_den.h
#include "chain_denom.h"
#include "chain_num.h"
#include "chain_xent.h"
#include "kf_prof.h"
#include "../../include/kf_ops.h"

#include <atomic>

KF_DECLARE_ERR(kfc)

extern "C" const char *kf_chain_last_error(void) { return kfc_err_.get(); }
extern "C" void kf_chain_clear_error(void) { kfc_err_.clear(); }

struct KfDenGraph {
    DenTables *t = nullptr;
    int num_arcs = 0;
    std::vector<float> init;
    float *d_init = nullptr;
    ~KfDenGraph() {
        delete t;
        if (d_init) hipFree(d_init);
    }
};

// Process-unique identity of a numerator batch's contents: kf_chain_compute's layout cache
// is keyed on it and not on the batch's address, which the allocator hands out again
// after a free (a new batch of the same shape would inherit the freed batch's
// descriptors). 0 is never drawn: it is the cache's "nothing cached".
static std::atomic<unsigned long long> g_num_batch_gen{0};
static unsigned long long next_num_batch_gen() { return ++g_num_batch_gen; }

struct KfNumBatch {
    NumDevice *nd = nullptr;
    std::vector<int> S;
    unsigned long long gen = next_num_batch_gen();  // redrawn by every refill
    // kf_num_batch_refill: device blob and its pinned host staging (grow only)
    int32_t *d_blob = nullptr;
    size_t d_cap = 0;                  // int32 entries
    int32_t *h_blob = nullptr;
    size_t h_cap = 0;
    hipEvent_t ev_copy = nullptr;      // the last refill's copy (h_blob is reused after it)
    ~KfNumBatch() {
        delete nd;
        if (ev_copy) {
            hipEventSynchronize(ev_copy);
            hipEventDestroy(ev_copy);
        }
        if (d_blob) hipFree(d_blob);
        if (h_blob) hipHostFree(h_blob);
    }
};

// What the cached layout of a KfChain was built from (re-uploaded only when it changes)
struct ChainLayoutKey {
    unsigned long long gen = 0;   // KfNumBatch::gen of the cached layout, 0 = none
    int nseq = 0, stride = -1;
    const void *nnet = nullptr;
    long long ld = -1, rows = -1;
    std::vector<int> row0, frames;
    bool matches(unsigned long long gen_, int nseq_, int stride_, const void *nnet_, long long ld_,
                 long long rows_, const int32_t *row0_, const int32_t *frames_) const {
        return gen == gen_ && nseq == nseq_ && stride == stride_ && nnet == nnet_ && ld == ld_ &&
               rows == rows_ && std::equal(row0_, row0_ + nseq_, row0.begin(), row0.end()) &&
               std::equal(frames_, frames_ + nseq_, frames.begin(), frames.end());
    }
};

struct KfChain {
    const KfDenGraph *den = nullptr;
    DenXBuf xbuf2;  // the backward recursion's exchange (k_den_fb)
    int max_seqs = 0, max_frames = 0;
    float *alpha_store = nullptr, *beta_store = nullptr, *asum_store = nullptr, *bsum_store = nullptr;
    float *stats = nullptr;
    float *h_stats = nullptr;     // pinned [max_seqs][8] (kf_chain_result)
    // kf_chain_xent (made at its first call): the per-frame objective terms [max_seqs][max_frames],
    // their pinned copy with the statistics behind it (kf_chain_xent_result), and whether
    // one ran since the last compute
    float *xent_part = nullptr, *h_xent = nullptr;
    bool xent_ran = false;
    float *num_ab = nullptr;      // numerator alpha/beta
    size_t num_ab_cap = 0;
    float *num_post = nullptr;    // sparse numerator posteriors
    size_t num_post_cap = 0;
    LogFstDev *d_desc = nullptr;  // [max_seqs]
    long long *d_row0 = nullptr;
    int *d_frames = nullptr;
    float *d_num_total = nullptr;
    // kf_chain_compute_weighted: [max_seqs] and [max_seqs][max_frames] behind the
    // frame counts, in the same allocation and staging slot; which of them the last compute
    // used (kf_chain_xent uses the same)
    float *d_seq_w = nullptr, *d_frame_w = nullptr;
    bool use_seq_w = false, use_frame_w = false;
    const float *grad_scale = nullptr;  // kf_chain_set_grad_scale: caller-owned device float, or off
    ChainLayoutKey last;         // cache of the last run's layout
    // pinned staging of the layout upload: two slots, each reused after its copy's event
    char *h_stage[2] = {nullptr, nullptr};
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    int stage_slot = 0;
    std::vector<LogFstDev> host_desc;
    size_t num_lds = 0;           // dynamic LDS of k_num_fb, 0 = use k_logfb
    float *den_out = nullptr;     // [max_seqs][2]
    hipStream_t side = nullptr;   // numerator stream (overlaps the den forward)
    hipEvent_t ev_in = nullptr, ev_num = nullptr;
    DenXBuf xbuf;
    unsigned long long *trace = nullptr;  // kf_chain_trace (diagnostics)
    int den_pairs = 1;                     // kf_chain_debug_den_pairs (tests)
    ~KfChain() {
        for (int i = 0; i < 2; ++i) {
            if (ev_stage[i]) {
                hipEventSynchronize(ev_stage[i]);
                hipEventDestroy(ev_stage[i]);
            }
            if (h_stage[i]) hipHostFree(h_stage[i]);
        }
        if (h_stats) hipHostFree(h_stats);
        if (h_xent) hipHostFree(h_xent);
        if (xent_part) hipFree(xent_part);
        if (side) hipStreamDestroy(side);
        if (ev_in) hipEventDestroy(ev_in);
        if (ev_num) hipEventDestroy(ev_num);
        if (den_out) hipFree(den_out);
        for (void *p : {(void *)alpha_store, (void *)beta_store, (void *)asum_store, (void *)bsum_store,
                        (void *)stats, (void *)num_ab,
                        (void *)num_post, (void *)d_desc, (void *)d_num_total})
            if (p) hipFree(p);
    }
};

extern "C" KfDenGraph *kf_den_graph_create(int S, int P, int A, const int32_t *src,
                                           const int32_t *dst, const int32_t *pdf0,
                                           const float *tp, int start_state,
                                           const float *initial_probs) {
    const char *why = nullptr;
    if (!src || !dst || !pdf0 || !tp || start_state < 0 || start_state >= S) {
        kfc_set_error("kf_den_graph_create: invalid arguments");
        return nullptr;
    }
    DenTables *t = make_den_tables(S, P, A, src, dst, pdf0, tp, &why);
    if (!t) {
        kfc_set_error("kf_den_graph_create: %s", why);
        return nullptr;
    }
    auto *g = new KfDenGraph();
    g->t = t;
    g->num_arcs = A;
    g->init.resize(S);
    if (initial_probs)
        memcpy(g->init.data(), initial_probs, S * 4);
    else
        compute_initial_probs(S, A, src, dst, tp, start_state, g->init.data());
    std::vector<void *> owned;
    g->d_init = dev_upload(g->init, owned);
    if (!g->d_init) {
        delete g;
        kfc_set_error("kf_den_graph_create: hipMalloc failed");
        return nullptr;
    }
    g->t->dev.init = g->d_init;
    den_tables_set_init(g->t->dev, g->d_init, kf_stream());
    if (hipStreamSynchronize(kf_stream()) != hipSuccess) {
        delete g;
        kfc_set_error("kf_den_graph_create: initial-probability gather failed");
        return nullptr;
    }
    return g;
}

extern "C" int kf_den_graph_initial_probs(const KfDenGraph *g, float *out) {
    if (!g || !out) return -1;
    memcpy(out, g->init.data(), g->init.size() * 4);
    return 0;
}
extern "C" void kf_den_graph_free(KfDenGraph *g) {
    kf_take_pending(__func__);
    delete g;
    kf_take_pending("the return of kf_den_graph_free");
}

// host CSR arrays (kf_chain.h layout) -> prepared numerator FSTs
static bool num_hosts(const char *fn, int nseq, const int32_t *state_off, const int32_t *arc_off,
                      const int32_t *row_ptr, const int32_t *dst, const int32_t *pdf1, const float *logw,
                      const int32_t *final_off, const int32_t *final_state, const float *final_logw,
                      std::vector<NumHost> &hs) {
    const char *why = nullptr;
    if (nseq <= 0 || !state_off || !arc_off || !row_ptr || !final_off) {
        kfc_set_error("%s: invalid arguments", fn);
        return false;
    }
    hs.assign(nseq, NumHost());
    for (int i = 0; i < nseq; ++i) {
        NumHost &h = hs[i];
        h.S = state_off[i + 1] - state_off[i];
        h.A = arc_off[i + 1] - arc_off[i];
        h.nfinal = final_off[i + 1] - final_off[i];
        h.start = 0;
        if (h.S <= 0 || h.A < 0 || h.nfinal < 0) {
            kfc_set_error("%s: sequence %d has an empty FST", fn, i);
            return false;
        }
        const int32_t *rp = row_ptr + state_off[i] + i;
        h.row_ptr.assign(rp, rp + h.S + 1);
        h.arc_dst.assign(dst + arc_off[i], dst + arc_off[i + 1]);
        h.arc_pdf.assign(pdf1 + arc_off[i], pdf1 + arc_off[i + 1]);
        h.arc_w.assign(logw + arc_off[i], logw + arc_off[i + 1]);
        h.fin_state.assign(final_state + final_off[i], final_state + final_off[i + 1]);
        h.fin_w.assign(final_logw + final_off[i], final_logw + final_off[i + 1]);
        if (!prepare_num(h, &why)) {
            kfc_set_error("%s: sequence %d: %s", fn, i, why);
            return false;
        }
    }
    return true;
}

extern "C" KfNumBatch *kf_num_batch_create(int nseq, const int32_t *state_off,
                                           const int32_t *arc_off, const int32_t *row_ptr,
                                           const int32_t *dst, const int32_t *pdf1,
                                           const float *logw, const int32_t *final_off,
                                           const int32_t *final_state, const float *final_logw) {
    const char *why = nullptr;
    std::vector<NumHost> hs;
    if (!num_hosts("kf_num_batch_create", nseq, state_off, arc_off, row_ptr, dst, pdf1, logw, final_off,
                   final_state, final_logw, hs))
        return nullptr;
    NumDevice *nd = upload_nums(hs, &why);
    if (!nd) {
        kfc_set_error("kf_num_batch_create: %s", why);
        return nullptr;
    }
    auto *b = new KfNumBatch();
    b->nd = nd;
    for (auto &h : hs) b->S.push_back(h.S);
    return b;
}

// TrainStep's per-minibatch numerator upload (chain_loss.go:44-97) without a device-wide
// stall: host preparation into pinned staging, one asynchronous copy on `stream` into
// buffers that only grow. The caller orders the copy after every kernel that still reads
// the batch's previous contents (e.g. `stream` waits for an event recorded after the
// kf_chain_compute that used it).
extern "C" int kf_num_batch_refill(KfNumBatch *b, int nseq, const int32_t *state_off,
                                   const int32_t *arc_off, const int32_t *row_ptr, const int32_t *dst,
                                   const int32_t *pdf1, const float *logw, const int32_t *final_off,
                                   const int32_t *final_state, const float *final_logw, void *stream) {
    if (!b) {
        kfc_set_error("kf_num_batch_refill: NULL batch");
        return -1;
    }
    std::vector<NumHost> hs;
    if (!num_hosts("kf_num_batch_refill", nseq, state_off, arc_off, row_ptr, dst, pdf1, logw, final_off,
                   final_state, final_logw, hs))
        return -1;
    std::vector<int32_t> blob;
    std::vector<std::vector<size_t>> offs;
    pack_nums(hs, blob, offs);
    const size_t n = std::max<size_t>(blob.size(), 4);
    hipStream_t st = stream ? (hipStream_t)stream : kf_stream();
    if (b->ev_copy) hipEventSynchronize(b->ev_copy);  // h_blob may still feed the last copy
    else if (hipEventCreateWithFlags(&b->ev_copy, hipEventDisableTiming) != hipSuccess) {
        kfc_set_error("kf_num_batch_refill: hipEventCreate failed");
        return -1;
    }
    if (n > b->h_cap) {
        if (b->h_blob) hipHostFree(b->h_blob);
        b->h_blob = nullptr;
        b->h_cap = 0;
        if (hipHostMalloc((void **)&b->h_blob, n * 4, 0) != hipSuccess) {
            kfc_set_error("kf_num_batch_refill: hipHostMalloc failed");
            return -1;
        }
        b->h_cap = n;
    }
    if (n > b->d_cap) {
        // growing: the old blob (this batch's own, or the create-time one) may still be
        // read by queued kernels; hipFree waits for the device
        if (b->d_blob) hipFree(b->d_blob);
        b->d_blob = nullptr;
        b->d_cap = 0;
        if (hipMalloc((void **)&b->d_blob, n * 4) != hipSuccess) {
            kfc_set_error("kf_num_batch_refill: hipMalloc failed");
            return -1;
        }
        b->d_cap = n;
    }
    if (b->nd && !b->nd->owned.empty()) {  // the create-time upload is no longer referenced
        hipDeviceSynchronize();
        for (void *p : b->nd->owned) hipFree(p);
        b->nd->owned.clear();
    }
    if (!b->nd) b->nd = new NumDevice();
    memcpy(b->h_blob, blob.data(), blob.size() * 4);
    if (hipMemcpyAsync(b->d_blob, b->h_blob, blob.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipEventRecord(b->ev_copy, st) != hipSuccess) {
        kfc_set_error("kf_num_batch_refill: copy failed");
        return -1;
    }
    num_descs(hs, offs, b->d_blob, b->nd);
    b->S.clear();
    for (auto &h : hs) b->S.push_back(h.S);
    b->gen = next_num_batch_gen();
    return 0;
}
extern "C" void kf_num_batch_free(KfNumBatch *b) {
    kf_take_pending(__func__);
    delete b;
    kf_take_pending("the return of kf_num_batch_free");
}

// bytes of the layout (descriptors, row offsets, frame counts) and of the whole staging slot,
// which carries the weights of a weighted compute behind it
static size_t layout_bytes(int max_seqs) { return (size_t)max_seqs * (sizeof(LogFstDev) + 12); }
static size_t slot_bytes(int max_seqs, int max_frames) {
    return layout_bytes(max_seqs) + (size_t)max_seqs * 4 + (size_t)max_seqs * max_frames * 4;
}

extern "C" KfChain *kf_chain_create(const KfDenGraph *den, int max_seqs, int max_frames) {
    if (!den || max_seqs <= 0 || max_frames <= 0) {
        kfc_set_error("kf_chain_create: invalid arguments");
        return nullptr;
    }
    auto *c = new KfChain();
    c->den = den;
    c->max_seqs = max_seqs;
    c->max_frames = max_frames;
    const int S = den->t->dev.S;
    const size_t rs = (size_t)den->t->dev.f.nsl * 64;  // slice-ordered state rows
    bool ok = hipMalloc(&c->alpha_store, (size_t)max_seqs * (max_frames + 1) * rs * 4) == hipSuccess;
    ok = ok && hipMalloc(&c->beta_store, (size_t)max_seqs * (max_frames + 1) * rs * 4) == hipSuccess;
    ok = ok && hipMalloc(&c->asum_store, (size_t)max_seqs * (max_frames + 1) * 4) == hipSuccess;
    ok = ok && hipMalloc(&c->bsum_store, (size_t)max_seqs * (max_frames + 1) * 4) == hipSuccess;
    ok = ok && hipMalloc(&c->stats, (size_t)max_seqs * 8 * 4) == hipSuccess;
    // descriptors, row offsets and frame counts in one allocation, laid out as the pinned
    // staging slot, so a layout change is one copy; the sequence and frame weights of a
    // weighted compute behind them
    ok = ok && hipMalloc(&c->d_desc, slot_bytes(max_seqs, max_frames)) == hipSuccess;
    if (ok) {
        c->d_row0 = reinterpret_cast<long long *>(reinterpret_cast<char *>(c->d_desc) + (size_t)max_seqs * sizeof(LogFstDev));
        c->d_frames = reinterpret_cast<int *>(reinterpret_cast<char *>(c->d_row0) + (size_t)max_seqs * 8);
        c->d_seq_w = reinterpret_cast<float *>(reinterpret_cast<char *>(c->d_desc) + layout_bytes(max_seqs));
        c->d_frame_w = c->d_seq_w + max_seqs;
    }
    ok = ok && hipMalloc(&c->d_num_total, (size_t)max_seqs * 4) == hipSuccess;
    ok = ok && hipMalloc(&c->den_out, (size_t)max_seqs * 8) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_num, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2; ++i) {
        ok = ok && hipEventCreateWithFlags(&c->ev_stage[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipHostMalloc((void **)&c->h_stage[i], slot_bytes(max_seqs, max_frames), 0) == hipSuccess;
    }
    if (!ok) {
        delete c;
        kfc_set_error("kf_chain_create: hipMalloc failed");
        return nullptr;
    }
    hipMemset(c->stats, 0, (size_t)max_seqs * 32);
    return c;
}
extern "C" void kf_chain_free(KfChain *c) {
    kf_take_pending(__func__);
    delete c;
    kf_take_pending("the return of kf_chain_free");
}

// ---- kf_chain_compute, step by step -----------------------------------------
static bool compute_args_ok(const KfChain *c, const KfNumBatch *num, const KfChainOpts *opts,
                            const void *nnet_output, long long ld, int nseq, const int32_t *seq_row0,
                            const int32_t *seq_frames, int stride, const void *out_grad, long long ldg,
                            const float *seq_w, const float *frame_w) {
    if (!c || !num || !opts || !nnet_output || !out_grad || !seq_row0 || !seq_frames) {
        kfc_set_error("kf_chain_compute: NULL argument");
        return false;
    }
    const int P = c->den->t->dev.P;
    if (nseq <= 0 || nseq > c->max_seqs || nseq != (int)num->nd->desc.size() || stride <= 0 ||
        ld < P || ldg < P) {
        kfc_set_error("kf_chain_compute: nseq %d (max %d, batch %zu), stride %d, ld %lld/%lld vs P %d",
                      nseq, c->max_seqs, num->nd->desc.size(), stride, ld, ldg, P);
        return false;
    }
    // every weight finite and >= 0 (0 is legal); the frame weights lie sequence after sequence
    for (int i = 0; seq_w && i < nseq; ++i)
        if (!(seq_w[i] >= 0.0f) || std::isinf(seq_w[i])) {
            kfc_set_error("kf_chain_compute_weighted: sequence %d: weight %g is not finite and >= 0", i, seq_w[i]);
            return false;
        }
    if (frame_w) {
        const float *fw = frame_w;
        for (int i = 0; i < nseq; fw += std::max(seq_frames[i], 0), ++i)
            for (int t = 0; t < seq_frames[i]; ++t)
                if (!(fw[t] >= 0.0f) || std::isinf(fw[t])) {
                    kfc_set_error("kf_chain_compute_weighted: sequence %d, frame %d: deriv weight %g is not "
                                  "finite and >= 0", i, t, fw[t]);
                    return false;
                }
    }
    return true;
}

// A new layout: range checks, the numerator buffers grown, the descriptors filled and
// uploaded with the row offsets and frame counts, the cache key set. The weights of a weighted
// compute ride in the same slot and copy (that compute comes here every time: the cache key
// does not cover them). False with the error set.
static bool layout_update(KfChain *c, const KfNumBatch *num, const void *nnet_output, long long ld,
                          long long num_rows, int nseq, const int32_t *seq_row0,
                          const int32_t *seq_frames, int stride, const float *seq_w, const float *frame_w,
                          hipStream_t st) {
    for (int i = 0; i < nseq; ++i)
        if (seq_frames[i] < 0 || seq_frames[i] > c->max_frames || seq_row0[i] < 0 ||
            (seq_frames[i] > 0 &&
             seq_row0[i] + (long long)(seq_frames[i] - 1) * stride >= num_rows)) {
            kfc_set_error("kf_chain_compute: sequence %d: %d frames (max %d), row0 %d, "
                          "stride %d outside %lld rows", i, seq_frames[i], c->max_frames,
                          seq_row0[i], stride, num_rows);
            return false;
        }
    size_t ab = 0, ps = 0;
    for (int i = 0; i < nseq; ++i) {
        ab += 2 * (size_t)(seq_frames[i] + 1) * num->S[i];
        ps += (size_t)seq_frames[i] * num->nd->G[i];
    }
    if ((ab > c->num_ab_cap && c->num_ab) || (ps > c->num_post_cap && c->num_post))
        hipDeviceSynchronize();  // growing: queued numerator kernels may still use the old buffers
    if (ab > c->num_ab_cap) {
        if (c->num_ab) hipFree(c->num_ab);
        c->num_ab = nullptr;
        if (hipMalloc(&c->num_ab, ab * 4) != hipSuccess) {
            c->num_ab_cap = 0;
            kfc_set_error("kf_chain_compute: hipMalloc failed");
            return false;
        }
        c->num_ab_cap = ab;
    }
    if (ps > c->num_post_cap) {
        if (c->num_post) hipFree(c->num_post);
        c->num_post = nullptr;
        if (hipMalloc(&c->num_post, std::max<size_t>(ps, 1) * 4) != hipSuccess) {
            c->num_post_cap = 0;
            kfc_set_error("kf_chain_compute: hipMalloc failed");
            return false;
        }
        c->num_post_cap = ps;
    }
    c->host_desc = num->nd->desc;
    float *ab_p = c->num_ab, *ps_p = c->num_post;
    std::vector<long long> r0(nseq);
    for (int i = 0; i < nseq; ++i) {
        LogFstDev &f = c->host_desc[i];
        f.T = seq_frames[i];
        f.mode = LF_FB | LF_POST;
        f.stride = stride;
        f.row0 = seq_row0[i];
        f.alpha = ab_p;
        ab_p += (size_t)(f.T + 1) * f.S;
        f.beta = ab_p;
        ab_p += (size_t)(f.T + 1) * f.S;
        f.post_sparse = ps_p;
        ps_p += (size_t)f.T * f.G;
        f.post_dense = nullptr;
        f.total = c->d_num_total + i;
        r0[i] = seq_row0[i];
    }
    c->num_lds = num_batch_lds(c->host_desc, num->nd->Ag, nseq);
    // asynchronous on st (every earlier reader of d_desc / d_row0 / d_frames is ahead of it
    // on st: the den kernels, and the numerator kernels through ev_num), from a pinned slot
    // whose previous copy has retired: no host stall when the batch changes every step
    const int slot = c->stage_slot;
    c->stage_slot ^= 1;
    hipEventSynchronize(c->ev_stage[slot]);
    char *hs_ = c->h_stage[slot];
    memcpy(hs_, c->host_desc.data(), nseq * sizeof(LogFstDev));
    memcpy(hs_ + (size_t)c->max_seqs * sizeof(LogFstDev), r0.data(), nseq * 8);
    memcpy(hs_ + (size_t)c->max_seqs * (sizeof(LogFstDev) + 8), seq_frames, nseq * 4);
    size_t nbytes = layout_bytes(c->max_seqs);
    if (seq_w || frame_w) {
        float *hw = reinterpret_cast<float *>(hs_ + nbytes);
        for (int i = 0; i < nseq; ++i) hw[i] = seq_w ? seq_w[i] : 1.0f;
        nbytes += (size_t)c->max_seqs * 4;
        if (frame_w) {  // [nseq][max_frames]; only a sequence's first frames[i] are read
            float *hf = hw + c->max_seqs;
            const float *fw = frame_w;
            for (int i = 0; i < nseq; fw += seq_frames[i], ++i)
                memcpy(hf + (size_t)i * c->max_frames, fw, (size_t)seq_frames[i] * 4);
            nbytes += (size_t)nseq * c->max_frames * 4;
        }
    }
    bool cp = hipMemcpyAsync(c->d_desc, hs_, nbytes, hipMemcpyHostToDevice, st) == hipSuccess;
    cp = cp && hipEventRecord(c->ev_stage[slot], st) == hipSuccess;
    if (!cp) {
        c->last.gen = 0;
        kfc_set_error("kf_chain_compute: layout upload failed");
        return false;
    }
    c->last.gen = num->gen;
    c->last.nseq = nseq;
    c->last.stride = stride;
    c->last.nnet = nnet_output;
    c->last.ld = ld;
    c->last.rows = num_rows;
    c->last.row0.assign(seq_row0, seq_row0 + nseq);
    c->last.frames.assign(seq_frames, seq_frames + nseq);
    return true;
}

// numerator on the side stream, overlapping the denominator forward; ev_num marks its end
static void launch_numerator(KfChain *c, const void *nnet_output, long long ld, int nseq,
                             const int32_t *seq_frames, hipStream_t st) {
    double num_arcs = 0;
    int maxT = 0;
    for (int i = 0; i < nseq; ++i) {
        num_arcs += (double)c->host_desc[i].A * seq_frames[i];
        maxT = std::max(maxT, seq_frames[i]);
    }
    hipEventRecord(c->ev_in, st);
    hipStreamWaitEvent(c->side, c->ev_in, 0);
    {
        hipStream_t saved = kf_stream();
        kf_set_stream((void *)c->side);
        int pn = kf_prof_start(KF_PROF_CHAIN_NUM, num_arcs);
        launch_num_batch(c->d_desc, (const h16 *)nnet_output, ld, c->den->t->dev.P, nseq, maxT, c->num_lds,
                         c->side);
        kf_prof_stop(pn);
        kf_set_stream((void *)saved);
    }
    hipEventRecord(c->ev_num, c->side);
}

// both den recursions in one launch, then (once the numerator is in) the posteriors and
// the objective assembly; false with the error set
static bool launch_denominator(KfChain *c, const KfChainOpts *opts, const void *nnet_output, long long ld,
                               int nseq, const int32_t *seq_frames, int stride, void *out_grad,
                               long long ldg, hipStream_t st) {
    double frames = 0;
    for (int i = 0; i < nseq; ++i) frames += seq_frames[i];
    DenRun r{};
    r.nnet = nnet_output;
    r.ld = ld;
    r.row0 = c->d_row0;
    r.frames = c->d_frames;
    r.stride = stride;
    r.max_frames = c->max_frames;
    r.leaky = opts->leaky_hmm_coefficient;
    r.backward = 1;
    r.alpha_store = c->alpha_store;
    r.beta_store = c->beta_store;
    r.asum_store = c->asum_store;
    r.bsum_store = c->bsum_store;
    r.stats = c->stats;
    r.den_out = c->den_out;
    r.trace = c->trace;
    r.nums = c->d_desc;
    r.out_grad = (h16 *)out_grad;
    r.ldg = ldg;
    r.opts = *opts;
    r.seq_w = c->use_seq_w ? c->d_seq_w : nullptr;
    r.frame_w = c->use_frame_w ? c->d_frame_w : nullptr;
    r.grad_scale = c->grad_scale;
    // algorithmic bytes: per frame three streamed passes over the
    // packed arc records, alpha' stored and re-read, the output row read twice
    // and the gradient row written once
    const DenDev &dd = c->den->t->dev;
    double bytes = frames * (3.0 * 8.0 * c->den->num_arcs + 8.0 * dd.S + 6.0 * dd.P);
    int pd = kf_prof_start(KF_PROF_CHAIN_DEN, bytes);
    DenX X{}, XB{};
    // forward and backward blocks share the CUs; sequence pairs (NS = 2) share each
    // record and gather when their interleaved rows fit the LDS
    const int ns = nseq >= 2 && dd.pair_ok && c->den_pairs ? 2 : 1;
    const int G = den_pick_G(2 * ((nseq + ns - 1) / ns));
    if (!c->xbuf.make(dd, dd.f, nseq, ns, G, X) || !c->xbuf2.make(dd, dd.b, nseq, ns, G, XB)) {
        kfc_set_error("kf_chain_compute: hipMalloc failed");
        return false;
    }
    launch_den_fb(dd, r, X, c->xbuf, XB, c->xbuf2, false);
    hipStreamWaitEvent(st, c->ev_num, 0);  // the numerator is needed from here on
    launch_den_post(dd, r, X, false, DEN_PRODUCT);
    kf_prof_stop(pd);
    return true;
}

extern "C" int kf_chain_compute_weighted(KfChain *c, const KfNumBatch *num, const KfChainOpts *opts,
                                         const void *nnet_output, long long ld, long long num_rows, int nseq,
                                         const int32_t *seq_row0, const int32_t *seq_frames, int stride,
                                         void *out_grad, long long ldg, const float *seq_weight,
                                         const float *frame_weight) {
    kf_take_pending(__func__);
    if (!compute_args_ok(c, num, opts, nnet_output, ld, nseq, seq_row0, seq_frames, stride, out_grad, ldg,
                         seq_weight, frame_weight))
        return -1;
    hipStream_t st = kf_stream();
    c->xent_ran = false;
    // a refilled numerator batch (kf_num_batch_refill): its copy lands before anything reads it
    if (num->ev_copy) hipStreamWaitEvent(st, num->ev_copy, 0);
    // weights change with every batch: a weighted compute uploads them (with the layout) every time
    const bool weighted = seq_weight || frame_weight;
    if ((weighted || !c->last.matches(num->gen, nseq, stride, nnet_output, ld, num_rows, seq_row0, seq_frames)) &&
        !layout_update(c, num, nnet_output, ld, num_rows, nseq, seq_row0, seq_frames, stride, seq_weight,
                       frame_weight, st))
        return -1;
    c->use_seq_w = seq_weight != nullptr;
    c->use_frame_w = frame_weight != nullptr;
    launch_numerator(c, nnet_output, ld, nseq, seq_frames, st);
    if (!launch_denominator(c, opts, nnet_output, ld, nseq, seq_frames, stride, out_grad, ldg, st)) return -1;
    if (hipGetLastError() != hipSuccess) {
        kfc_set_error("kf_chain_compute: launch failed");
        return -1;
    }
    return 0;
}

extern "C" int kf_chain_compute(KfChain *c, const KfNumBatch *num, const KfChainOpts *opts,
                                const void *nnet_output, long long ld, long long num_rows, int nseq,
                                const int32_t *seq_row0, const int32_t *seq_frames, int stride,
                                void *out_grad, long long ldg) {
    return kf_chain_compute_weighted(c, num, opts, nnet_output, ld, num_rows, nseq, seq_row0, seq_frames, stride,
                                     out_grad, ldg, nullptr, nullptr);
}

// The xent output's derivative and objective (chain_xent.hip) over the layout and the numerator
// posteriors of the compute before it, on the same stream: the posteriors, the descriptors and
// the statistics' ok are ahead of it there (kf_chain_compute joined the numerator stream).
extern "C" int kf_chain_xent(KfChain *c, const KfNumBatch *num, const KfChainOpts *opts, const void *xent_output,
                             long long ldx, void *xent_grad, long long ldg) {
    kf_take_pending(__func__);
    if (!c || !num || !opts || !xent_output || !xent_grad) {
        kfc_set_error("kf_chain_xent: NULL argument");
        return -1;
    }
    if (c->last.gen == 0) {
        kfc_set_error("kf_chain_xent: no kf_chain_compute before it");
        return -1;
    }
    if (num->gen != c->last.gen || (int)num->nd->desc.size() != c->last.nseq) {
        kfc_set_error("kf_chain_xent: the numerator batch is not the one of the last kf_chain_compute");
        return -1;
    }
    const int P = c->den->t->dev.P, nseq = c->last.nseq;
    if (ldx < P || ldg < P) {
        kfc_set_error("kf_chain_xent: ldx %lld / ldg %lld below P %d", ldx, ldg, P);
        return -1;
    }
    if (!c->xent_part) {
        const size_t n = (size_t)c->max_seqs * c->max_frames;
        if (hipMalloc(&c->xent_part, n * 4) != hipSuccess ||
            hipHostMalloc((void **)&c->h_xent, (n + (size_t)c->max_seqs * 8) * 4, hipHostMallocDefault) != hipSuccess) {
            if (c->xent_part) hipFree(c->xent_part);
            c->xent_part = nullptr;
            c->h_xent = nullptr;
            kf_take_pending("kf_chain_xent allocation");
            kfc_set_error("kf_chain_xent: allocation failed");
            return -1;
        }
    }
    XentRun r{};
    r.nums = c->d_desc;
    r.row0 = c->d_row0;
    r.frames = c->d_frames;
    r.stats = c->stats;
    r.y = (const h16 *)xent_output;
    r.ldx = ldx;
    r.grad = (h16 *)xent_grad;
    r.ldg = ldg;
    r.part = c->xent_part;
    r.part_ld = c->max_frames;
    r.P = P;
    r.stride = c->last.stride;
    r.w = opts->supervision_weight;
    r.scale = opts->xent_regularize * opts->supervision_weight;
    // after a weighted compute: its weights, still on the device
    r.xr = opts->xent_regularize;
    r.seq_w = c->use_seq_w ? c->d_seq_w : nullptr;
    r.frame_w = c->use_frame_w ? c->d_frame_w : nullptr;
    r.grad_scale = c->grad_scale;
    double frames = 0;
    for (int f : c->last.frames) {
        frames += f;
        r.max_t = std::max(r.max_t, f);
    }
    launch_chain_xent(r, nseq, frames);
    if (hipGetLastError() != hipSuccess) {
        kfc_set_error("kf_chain_xent: launch failed");
        return -1;
    }
    c->xent_ran = true;
    return 0;
}

extern "C" void kf_chain_set_grad_scale(KfChain *c, const float *scale_dev) {
    if (c) c->grad_scale = scale_dev;
}

// Synchronises; the per-frame terms of every sequence summed in double, frame by frame and
// sequence by sequence (a fixed order), and the weights the chain statistics count.
extern "C" int kf_chain_xent_result(KfChain *c, double *xent_objf, double *total_weight) {
    if (!c) {
        kfc_set_error("kf_chain_xent_result: NULL argument");
        return -1;
    }
    kf_take_pending(__func__);
    if (!c->xent_ran) {
        kfc_set_error("kf_chain_xent_result: no kf_chain_xent since the last kf_chain_compute");
        return -1;
    }
    const int n = c->last.nseq;
    const size_t np = (size_t)c->max_seqs * c->max_frames;
    hipStream_t st = kf_stream();
    // (one copy of the first n sequences' rows; only the frames the kernel wrote are read below)
    bool ok = hipMemcpyAsync(c->h_xent, c->xent_part, (size_t)n * c->max_frames * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(c->h_xent + np, c->stats, (size_t)n * 8 * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
    if (!ok || hipStreamSynchronize(st) != hipSuccess) {
        kf_take_pending("kf_chain_xent_result copy");
        kfc_set_error("kf_chain_xent_result: copy failed");
        return -1;
    }
    double objf = 0.0, wsum = 0.0;
    for (int i = 0; i < n; ++i) {
        double o = 0.0;
        for (int t = 0; t < c->last.frames[i]; ++t) o += c->h_xent[(size_t)i * c->max_frames + t];
        objf += o;
        wsum += c->h_xent[np + (size_t)i * 8 + 4];
    }
    if (xent_objf) *xent_objf = objf;
    if (total_weight) *total_weight = wsum;
    return 0;
}

// Diagnostics: when `buf` (device, 32*8 + 32*2*16 u64) is non-null, the den forward
// kernel of sequence 0 / block 0 records 8 phase timestamps (wall_clock64, 100 MHz) for
// frames 16..47 of every later compute, then the arc-phase end of every wave of blocks
// 0 and 1 of sequence 0. Not part of the product contract.
extern "C" void kf_chain_trace(KfChain *c, unsigned long long *buf) {
    if (c) c->trace = buf;
}

// diagnostics (tests): polls an exchange wait makes before it gives up; 0 forces the
// timeout path on the first wait that is not already satisfied. 0xFFFFFFFF = default.
extern "C" void kf_chain_debug_spin_limit(KfChain *c, unsigned polls) {
    if (!c) return;
    const unsigned v = polls == 0xFFFFFFFFu ? (1u << 21) : polls;
    c->xbuf.spin_limit = c->xbuf2.spin_limit = v;
}

// diagnostics (tests): 0 runs the den recursions one sequence per unit (NS = 1) even
// where sequence pairs fit; 1 = default
extern "C" void kf_chain_debug_den_pairs(KfChain *c, int pairs) {
    if (c) c->den_pairs = pairs ? 1 : 0;
}

// diagnostics (tests): 1 makes the den exchange use agent scope (sc1 through to memory)
// even where the blocks of a sequence share an XCD; 0 = default (L2-local when they do)
extern "C" void kf_chain_debug_exchange_sys(KfChain *c, int force) {
    if (c) c->xbuf.force_sys = c->xbuf2.force_sys = force ? 1 : 0;
}

// diagnostics (tests): the XCD census of the last compute's den launch. *units = exchange
// units per direction, *G = workgroups per unit; *local_fwd / *local_bwd = units whose G
// workgroups all ran on one XCD, i.e. took the L2-local exchange unless
// kf_chain_debug_exchange_sys forced agent scope (*forced = 1). 0, or -1 on error.
extern "C" int kf_chain_debug_census(KfChain *c, int *units, int *local_fwd, int *local_bwd, int *forced, int *G) {
    if (!c) return -1;
    hipStream_t st = kf_stream();
    const int f = c->xbuf.census_local(st), b = c->xbuf2.census_local(st);
    if (f < 0 || b < 0) {
        kfc_set_error("kf_chain_debug_census: read failed");
        return -1;
    }
    if (units) *units = c->xbuf.last_units;
    if (local_fwd) *local_fwd = f;
    if (local_bwd) *local_bwd = b;
    if (forced) *forced = c->xbuf.force_sys;
    if (G) *G = c->xbuf.last_G;
    return 0;
}

extern "C" const float *kf_chain_seq_stats(const KfChain *c) { return c ? c->stats : nullptr; }

extern "C" int kf_chain_result(KfChain *c, KfChainResult *out) {
    if (!c || !out) return -1;
    kf_take_pending("kf_chain_result");
    const int n = c->last.nseq;
    hipStream_t st = kf_stream();
    // pinned staging (a stream-ordered copy into pageable memory left a spurious
    // hipErrorStreamCaptureUnsupported pending on the calling thread)
    if (n && !c->h_stats &&
        hipHostMalloc((void **)&c->h_stats, (size_t)c->max_seqs * 8 * 4, hipHostMallocDefault) != hipSuccess) {
        c->h_stats = nullptr;
        kf_take_pending("kf_chain_result hipHostMalloc");
        kfc_set_error("kf_chain_result: pinned staging allocation failed");
        return -1;
    }
    if (n && hipMemcpyAsync(c->h_stats, c->stats, (size_t)n * 8 * 4, hipMemcpyDeviceToHost, st) != hipSuccess) {
        kf_take_pending("kf_chain_result hipMemcpyAsync");
        kfc_set_error("kf_chain_result: statistics copy failed");
        return -1;
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
        kf_take_pending("kf_chain_result hipStreamSynchronize");
        kfc_set_error("kf_chain_result: stream error");
        return -1;
    }
    kf_take_pending("kf_chain_result after the statistics copy");
    const float *s = c->h_stats;
    // every compute since the last result: the sticky count is never reset by a launch
    if (const unsigned nt = c->xbuf.take_timeouts(st) + c->xbuf2.take_timeouts(st)) {
        kfc_set_error("kf_chain_result: den cross-workgroup exchange timed out in %u block(s) since the last "
                      "result (blocks not resident); the objective and gradients of those computes are invalid",
                      nt);
        return -1;
    }
    memset(out, 0, sizeof(*out));
    for (int i = 0; i < n; ++i) {
        const float *v = &s[(size_t)i * 8];
        out->num_logprob += v[0];
        out->den_logprob += v[1];
        out->objf += v[2];
        out->l2_term += v[3];
        out->total_weight += v[4];
        out->frames += (int)v[5];
        out->out_of_range += (int)v[6];
        out->num_ok += v[7] > 0.5f;
    }
    out->num_seqs = n;
    return 0;
}
