// backward.cpp — the backward pass of the C++ host layer (Network.Backward,
// network_backward.go:94-143): exact gradients of forward.cpp's launches. BackwardPass owns
// the streams and the gradient ring; one member function per layer kind does the launches.
#include <climits>
#include <cstdlib>

#include "net_internal.h"

namespace {

// ring index of an input-gradient buffer, or -1
int dz_index(const KfNet *net, const void *p) {
    for (int i = 0; i < 3; ++i)
        if (p == net->dz[i]) return i;
    return -1;
}

// Epilogue of an input-gradient GEMM that produces the gradient of layer P
// (the input of the layer being back-propagated). v = acc (+ bypass * g_cur):
//   g_P = rne(v) when P itself has a bypass (its own input gradient needs it)
//   dz_P = rne(v * bnscale_P * mask_P) for relu+BN layers, rne(v*bn2scale) for prefinal
// A TDNN-F P whose forward applied a dropout mask: dz_P = rne(v * bnscale_P * drop_P * mask_P),
// the table P's own (not that of the layer being back-propagated); g_P is not masked, the
// bypass went round the dropout. compact_rows: the producing GEMM's rows are the compact row set.
bool dx_epilogue(KfNet *net, int P, void *dz_out, void *g_out, KfEpilogue &E, bool compact_rows) {
    E = epi0();
    NetLayer &pl = net->layers[P];
    const Layer &L = pl.L;
    const int w = L.out_dim;
    E.ldo2 = w;
    E.out2 = dz_out;
    const int di = dz_index(net, dz_out);
    if (di >= 0) net->dz_imp[di] = net->dz_edge[di] = false;
    switch (L.type) {
        case LayerType::TDNNF: {
            if (pl.bnt_act) {
                // training-mode BatchNorm: the raw g only, bypass or not (the g ring
                // is as wide as the widest layer); P's own step turns it into dz, through the
                // batch statistics (BackwardPass::tdnnf). dz_edge stays false: that step's
                // kf_rows_sum_mask sums the strided layers' edge row.
                E.out = g_out;
                E.ldo = w;
                E.out2 = nullptr;
                return true;
            }
            E.scale2 = pl.bn_scale;
            E.mask_in = pl.mask;
            if (pl.drop_act) {
                E.drop = pl.drop;
                E.ld_drop = w;
                E.row_seg = drop_rows(net, compact_rows);
            }
            if (pl.bypass) {
                E.out = g_out;
                E.ldo = w;
                // implicit dz: g is stored anyway, its consumers apply mask and scale (the
                // masked weight gradient needs 256-column tiles: w > 128, not 160 / 320)
                const bool shape_ok = w > 128 && !(w % 160 == 0 && w <= 320);
                if (net->implicit_dz && !net->fp8 && di >= 0 && pl.mask && pl.bn_scale && net->w2s && shape_ok) {
                    E.out2 = nullptr;
                    E.scale2 = nullptr;
                    E.mask_in = nullptr;
                    net->dz_imp[di] = true;
                    return true;
                }
            }
            // a strided P's clamped-splice edge row (row T of dz: sum of its rows T-1-s .. T-1),
            // summed by the epilogue's last row tile instead of a separate kf_rows_sum launch
            if (L.time_stride > 0 && di >= 0 && net->T > 0 && !(net->rs.Tc && pl.compact)) {
                const int T = net->T;
                E.edge_out = (char *)dz_out + (size_t)T * w * 2;
                E.edge_r0 = T - 1 - L.time_stride < 0 ? 0 : T - 1 - L.time_stride;
                E.edge_r1 = T;
                E.edge_src = 1;
                net->dz_edge[di] = true;
            }
            // MXFP8 train step: also the e4m3 copy of dz_P for P's affine input gradient; only
            // when the copy's row is exactly w wide (w % 128 == 0), so the dgrad GEMM's K range
            // holds no stale codes from a wider layer's copy
            if (net->fp8 && net->fp8_dgrad && di >= 0 && w % 128 == 0 && pl.w8d.q && net->dz8[di].q &&
                net->dz8[di].ld == w) {
                E.out8 = net->dz8[di].q;
                E.ldo8 = net->dz8[di].ld;
                E.scale8 = net->dz8[di].s;
                E.out8_src = 1;
                net->dz8_layer[di] = P;
            }
            return true;
        }
        case LayerType::ConvReluBN:
            if (pl.bnt_act) {
                // training-mode BatchNorm: the raw g only, through out2 (every conv
                // input-gradient path writes there) into the g ring; P's own step makes dz of it
                // in the ring slot left unwritten here (BackwardPass::conv)
                E.out2 = g_out;
                return true;
            }
            [[fallthrough]];
        case LayerType::Attention:
            E.scale2 = pl.bn_scale;
            E.mask_in = pl.mask;
            return true;
        case LayerType::Prefinal:
            if (pl.bnt_act && pl.has_bn2) {  // as for conv: BatchNorm 1's backward is P's own step's
                E.out2 = g_out;
                return true;
            }
            if (pl.has_bn2) E.scale2 = pl.bn2_scale;
            return true;
        case LayerType::Batchnorm:
            // batchnorm-component (frozen statistics): the gradient at its input is the
            // output gradient times its per-column scale (backward_wrappers.cu:105-115),
            // applied in the producing GEMM's epilogue; the step through the BN layer is
            // then a pass-through (BackwardPass::step). Its own input must take a raw gradient.
            if (pl.input < 0 || !(net->layers[pl.input].L.type == LayerType::Linear)) {
                set_err("backward: gradient through batchnorm-component " + L.name +
                        " into a layer other than linear-component is not supported");
                return false;
            }
            E.scale2 = pl.bn_scale;
            return true;
        case LayerType::Linear:
        case LayerType::CombineFeatureMaps:  // raw gradient; its backward splits it (ivector branch)
            return true;
        default:
            set_err("backward: gradient into layer " + L.name + " is not supported");
            return false;
    }
}

// issue every bucket planned to follow backward step `step` (INT_MAX: all left)
bool dp_issue(KfNet *net, size_t &next, int step) {
    for (; next < net->dp_after.size() && net->dp_after[next] <= step; ++next)
        if (kf_dp_allreduce_mean_async(net->dp, net->grad + net->dp_begin[next],
                                       (size_t)(net->dp_end[next] - net->dp_begin[next])) != 0) {
            const char *e = kf_dp_last_error();
            set_err(std::string("dp all-reduce: ") + (e ? e : ""));
            return false;
        }
    return true;
}

// conv input gradient with the weights as a plain [taps * fout x fin] B, N contiguous (the
// forward's B layout): block i = (tap taps[i]'s fin rows of W)^T, one batched transpose per
// layer and step. The shifted k-contiguous weight rows (op_wrows, the BROW halo kernels) ran
// cnn4's input gradient at half the forward's rate. KF_DGRAD_WT=0: op_wrows. The K order is
// the same either way, so the result is bit-identical.
bool dgrad_wt_on() {
    const char *e = getenv("KF_DGRAD_WT");
    return !(e && e[0] == '0');
}
void *dgrad_wt(KfNet *net, NetLayer &nl, const std::vector<int> &taps) {
    const Layer &L = nl.L;
    const size_t blk = (size_t)L.fin * L.fout * 2;
    if ((int)taps.size() > KF_TRANSPOSE_MAX || taps.size() > nl.dt.size()) return nullptr;
    if (!nl.wtd) nl.wtd = net->dalloc(nl.dt.size() * blk);
    if (!nl.wtd) return nullptr;
    std::vector<const void *> src;
    std::vector<void *> dst;
    std::vector<int> M, N;
    for (size_t i = 0; i < taps.size(); ++i) {
        src.push_back((const char *)wptr(net, nl.pW) + taps[i] * blk);
        dst.push_back((char *)nl.wtd + i * blk);
        M.push_back(L.fin);
        N.push_back(L.fout);
    }
    if (kf_transpose_batch((int)taps.size(), src.data(), dst.data(), M.data(), N.data()) != 0) return nullptr;
    return nl.wtd;
}

// E at input frame f of a conv layer's input gradient viewed as [(t,h) x fin]
KfEpilogue at_frame(const KfEpilogue &E, const Layer &L, long long f) {
    const long long off = f * L.hin * L.fin;
    KfEpilogue X = E;
    X.ldo2 = L.fin;
    X.out2 = (char *)E.out2 + off * 2;
    if (E.out) {
        X.ldo = L.fin;
        X.out = (char *)E.out + off * 2;
    }
    if (E.mask_in) X.mask_in = E.mask_in + off / 8;
    if (E.mask_out) X.mask_out = E.mask_out + off / 8;
    return X;
}

// one layer's backward step
struct Step {
    NetLayer &nl;
    int li;
    int T, Tfull;       // the layer's rows (compact above the conv stack, row subsampling) / the forward's
    const void *x;      // the layer's input, as its forward read it
    bool want_dx;       // a trainable layer lies below
    bool to_full;       // the first compact layer: its input gradient is scattered to full rows
    void *dz_next, *g_next, *dbott_buf;
    KfEpilogue E;       // of the GEMM that produces the input gradient (dx_epilogue)
};
// a TDNN-F step's shapes and buffers
struct Tdnnf {
    int s, bn, klin, kaff;
    int ib;             // ring index of dz, or -1
    bool imp;           // implicit dz (dx_epilogue): the layer's g read through its ReLU mask, the BN
    const void *dzs;    //   scale applied to the weight gradient's columns and folded into W2
    const void *w2;
    void *dbott;
};

// Two streams: the input-gradient chain on the caller's stream (main), every write into
// the gradient buffer on the weight-gradient stream (side), which waits for main at each
// wgrad(): the dW GEMMs of a layer overlap the input gradients below it. Hazards (WAR on
// shared scratch) are ordered by events: the dz / g / dbott buffers cycle three deep and
// main waits for a step's side work before it overwrites what that work read (dx_wait,
// side_wait). All gradient writes (and so the data-parallel
// bucket gates, dp_issue) are on side; main joins side before returning.
struct BackwardPass {
    KfNet *const net;
    void *const caller;  // the stream current at entry; every return leaves it current
    void *mainst;
    const bool two;
    // With the weight-gradient stream the input-gradient chain runs on a high-priority
    // stream (its workgroups are dispatched ahead of the weight gradients') and each weight
    // gradient launches 256 workgroups instead of 512. Same-box A/B (bench default, 20
    // steps, median): one stream 38.13 / 38.36 ms, two streams 37.57 / 37.52;
    // the chain's priority is neutral (37.55 without it), 512-workgroup weight gradients
    // cost 1.2 ms (38.78). With the row-subsampled step (r6) 160 workgroups: non-den step
    // time 17.52 ms against 17.81 at 256, 17.57 at 128, 18.15 at 96 (same box, 3 runs each).
    const bool hp;
    const int old_target;
    // Steps (layers that hand a gradient down) cycle through three dz / g / dbott buffers.
    // Before step i rewrites its dz / g buffers, main waits for the side work of step i - 2,
    // the last reader of what step i - 3 wrote there; before it rewrites its dbott buffer
    // (earlier in the step), for that of step i - 3. Step i - 1's side work keeps running.
    // The side stream is in order, so waiting for step j's event covers every step <= j.
    int stepi = 0, waited = -1;  // side work of steps <= waited: main has waited for it
    int flip = 0, done = 0;
    // dbott cycles by TDNN-F / prefinal step (the steps that write it), not by layer: a
    // pass-through step in between (Batchnorm) must not advance it, or the next step would
    // reuse a buffer whose weight gradient may still read it (side_wait covers step i - 3).
    int nbott = 0;
    size_t dp_next = 0;
    const void *dz;    // gradient w.r.t. pre-activation of the current layer
    const void *gcur;  // stored gradient w.r.t. the current layer's output
    // nnet_backward_xent: the xent branch's layers from its output down (NULL: a
    // chain-only backward), the branch point's width, and the chain-path layer that reads the
    // branch point. The branch's last step writes its input gradient to net->gx instead of the
    // dz ring; the join layer's input-gradient epilogue adds it through the residual slot.
    const std::vector<int> *branch = nullptr;
    int branch_dim = 0, join_li = -1;

    // (the top layer must be the chain output)
    BackwardPass(KfNet *n, const void *out_grad)
        : net(n), caller(kf_get_stream()), mainst(caller), two(n->wg_side != 0 && n->wg_stream != nullptr),
          hp(two && n->hp_stream), old_target(kf_gemm_wgrad_target(two ? 160 : 0)), dz(out_grad), gcur(out_grad) {}
    ~BackwardPass() {
        kf_gemm_wgrad_target(old_target);
        kf_set_stream(caller);
    }

    bool to_side() {  // side continues after everything main enqueued so far
        if (!two) return true;
        if (kf_event_record(net->ev_go, mainst) != 0 || kf_stream_wait(net->wg_stream, net->ev_go) != 0) {
            set_err("backward: weight-gradient stream order");
            return false;
        }
        kf_set_stream(net->wg_stream);
        if (net->stall_side > 0 && kf_debug_spin(net->wg_stream, net->stall_side) != 0) {
            set_err("backward: debug stall");
            return false;
        }
        return true;
    }
    void to_main() { kf_set_stream(mainst); }
    bool side_wait(int upto) {
        if (!two || upto <= waited || upto < 0) return true;
        if (kf_stream_wait(mainst, net->ev_step[upto % 3]) != 0) {
            set_err("backward: weight-gradient stream join");
            return false;
        }
        waited = upto;
        return true;
    }
    bool dx_wait() { return side_wait(stepi - 2); }
    // main waits for everything on side so far
    bool join_side() {
        if (!two || (kf_event_record(net->ev_side, net->wg_stream) == 0 && kf_stream_wait(mainst, net->ev_side) == 0))
            return true;
        set_err("backward: weight-gradient stream join");
        return false;
    }
    // a weight gradient: on side, after what main enqueued so far
    template <class F>
    bool wgrad(F &&f) {
        if (!to_side()) return false;
        const bool ok = f();
        to_main();
        return ok;
    }

    // natural gradient: a component's statistics, issued where its weight gradient
    // is, on the same stream and over the same operands
    bool ng_stats(int pW, const KfOperand &X, const KfOperand &dY, int T);
    bool ng_side(const KfNgPre &p, const KfOperand &X, bool ones, int T);
    bool ng_finish();

    bool begin();
    bool branch_pass(const void *xent_grad, const void *out_grad);
    int step(int li, int ndone);  // 1: go on below, 0: nothing trainable below, -1: failed
    bool finish();

    // one function per layer kind; TDNN-F and conv split by what they launch
    bool to_full_epilogue(Step &s), to_full_scatter(Step &s);
    bool linear(Step &s), attention(Step &s), prefinal(Step &s), combine(Step &s), tdnnf(Step &s), conv(Step &s);
    KfOperand masked(const Step &s, const Tdnnf &t, KfOperand o) const;
    bool bn_train_dz(Step &s, int ib);
    bool bn_rows_entries();
    bool bn_site_dz(const void *g, const void *r, int rows, int stat_rows, int H, int F, const float *stat, float rms,
                    const uint8_t *mask, void *dz_out, const std::string &what, const float *repair = nullptr);
    bool repair_vectors();
    void *bn_site_slot(const NetLayer &nl);
    bool tdnnf_affine_wgrad(Step &s, const Tdnnf &t), tdnnf_affine_dgrad(Step &s, const Tdnnf &t);
    bool tdnnf_affine_dgrad_mx(Step &s, const Tdnnf &t, const KfEpilogue &E1, void *edge);
    bool tdnnf_linear_wgrad(Step &s, const Tdnnf &t), tdnnf_linear_dgrad(Step &s, const Tdnnf &t);
    bool conv_small_fin(Step &s), conv_wgrad_plain(Step &s), conv_wgrad_compact(Step &s);
    bool conv_window(Step &s, bool side);
    bool conv_dgrad_compact(Step &s), conv_dgrad_strided(Step &s), conv_dgrad_plain(Step &s);
};

// One side's statistics of a minibatch X [T x D] (kf_ops.h): trX and N, H = X W^T in fp16 (the
// bias epilogue adds the ones column's term), L = H^T H, and on an updating step JT = X^T H
// (its bias row: the ones column's). H is one buffer: the stream is in order.
bool BackwardPass::ng_side(const KfNgPre &p, const KfOperand &X, bool ones, int T) {
    const int Rp = (p.R + 31) / 32 * 32, K = X.ncols, ldh = KF_NG_W16_LD(p.D);
    float *st = net->ng_stat + p.st_off;
    const char *wh = (const char *)net->ng_w16 + p.h_off * 2;
    if (X.mask || K + (ones ? 1 : 0) != p.D) {
        set_err("natural gradient: a masked operand (implicit dz) or a shape that does not match the table");
        return false;
    }
    if (!ck(kf_ng_trx(&X, ones ? 1 : 0, st), "natural gradient trX")) return false;
    KfOperand Xk = X;
    Xk.kcontig = 1;
    KfOperand Wb = op_base(wh, ldh, Rp, K, 1);
    KfEpilogue E = epi0();
    E.out = net->ng_h;
    E.ldo = Rp;
    if (ones) E.bias = wh + (size_t)Rp * ldh * 2;
    if (!ck(kf_gemm_fused(T, Rp, K, &Xk, &Wb, &E), "natural gradient H")) return false;
    KfOperand H = op_base(net->ng_h, Rp, T, Rp, 0);
    if (!ck(kf_gemm_wgrad(Rp, Rp, T, &H, &H, st + KF_NG_STAT_L, Rp, nullptr, 0), "natural gradient L")) return false;
    if (!net->ng_updating) return true;
    float *jt = st + KF_NG_STAT_JT(Rp);
    return ck(kf_gemm_wgrad(K, Rp, T, &X, &H, jt, Rp, ones ? jt + (size_t)K * Rp : nullptr, 0), "natural gradient J");
}

bool BackwardPass::ng_stats(int pW, const KfOperand &X, const KfOperand &dY, int T) {
    if (!net->ng_on || pW < 0 || net->ng_of_param[pW] < 0) return true;
    const int ci = net->ng_of_param[pW];
    const KfNgComp &c = net->ng_comps[ci];
    if (c.pre_in >= 0 && !ng_side(net->ng_pres[c.pre_in], X, c.db_off >= 0, T)) return false;
    if (c.pre_out >= 0 && !ng_side(net->ng_pres[c.pre_out], dY, false, T)) return false;
    net->ng_issued[ci] = 1;
    return true;
}

// after the weight-gradient stream is joined: the batched scales, apply and state launches
bool BackwardPass::ng_finish() {
    if (!net->ng_on || net->ng_comps.empty()) return true;
    for (size_t i = 0; i < net->ng_comps.size(); ++i)
        if (!net->ng_issued[i]) {
            set_err("natural gradient: a preconditioned component got no weight gradient in this backward");
            return false;
        }
    const KfNgPre *pres = net->ng_pres.data(), *pres_dev = (const KfNgPre *)net->ng_pres_dev;
    const int npre = (int)net->ng_pres.size(), ncomp = (int)net->ng_comps.size();
    if (!ck(kf_ng_scales(pres, pres_dev, npre, &net->ng_opts, net->ng_sc, net->ng_stat, net->ng_report), "natural gradient scales") ||
        !ck(kf_ng_apply(net->grad, net->nparams, net->ng_comps.data(), (const KfNgComp *)net->ng_comps_dev, ncomp, pres,
                        pres_dev, npre, net->ng_w32, net->ng_report, net->ng_apply_scratch),
            "natural gradient apply") ||
        !ck(kf_ng_state(pres, pres_dev, npre, &net->ng_opts, net->ng_updating ? 1 : 0, net->ng_w32, net->ng_w16, net->ng_sc,
                        net->ng_stat, net->ng_state_scratch, net->ng_report),
            "natural gradient state"))
        return false;
    ++net->ng_t;
    net->ng_ran = true;
    return true;
}

bool BackwardPass::begin() {
    if (net->ng_on) {
        if (net->implicit_dz || net->fp8 || net->dp || (two && net->main_aff > 0)) {
            set_err("natural gradient: not supported with implicit dz, MXFP8, data parallel or nnet_debug_backward's "
                    "main_aff");
            return false;
        }
        std::fill(net->ng_issued.begin(), net->ng_issued.end(), 0);
        net->ng_updating = net->ng_t < 10 || net->ng_t % net->ng_opts.update_period == 0;
    }
    if (hp) {
        if (kf_event_record(net->ev_go, caller) != 0 || kf_stream_wait(net->hp_stream, net->ev_go) != 0) {
            set_err("backward: chain stream order");
            return false;
        }
        mainst = net->hp_stream;
        kf_set_stream(mainst);
    }
    if (!to_side()) return false;
    // (the xent branch's weight gradients overwrite their ranges: nnet_backward_xent zeroes the rest)
    auto branch_writes = [&](long long off) {
        if (!branch) return false;
        for (int li : *branch) {
            const NetLayer &q = net->layers[li];
            for (int pi : {q.pW, q.pb, q.pW2, q.pb2})
                if (pi >= 0 && net->params[pi].off == off) return true;
        }
        return false;
    };
    for (const auto &r : net->offpath)
        if (!branch_writes(r.first)) bridge_gpu_memset(net->grad + r.first, 0, (size_t)r.second * 4);
    // negative control of the data-parallel tests: exchanging before any producer ran
    if (net->dp && net->dp_early) {
        if (!dp_issue(net, dp_next, INT_MAX)) return false;
        // ... and finished before any producer writes (deterministic: left to race with the
        // backward, a fast one could finish first and hide the early exchange)
        if (kf_dp_join(net->dp) != 0 ||
            (two && (kf_event_record(net->ev_side, net->wg_stream) != 0 || kf_stream_wait(mainst, net->ev_side) != 0))) {
            set_err("backward: early-exchange join");
            return false;
        }
    }
    to_main();
    // the bottleneck-gradient row mask of this row set (rebuilt when the set changes, on the
    // chain stream, which reads it): every 3-strided compact TDNN-F layer of one bottleneck
    // width zeroes the scratch row through it
    if (net->rs.Tc > net->rs.Tc0 && net->rowmask) {
        int bn = 0;
        for (size_t li = net->first_c; li < net->layers.size(); ++li) {
            const Layer &q = net->layers[li].L;
            if (q.type != LayerType::TDNNF || q.time_stride == 0) continue;
            bn = bn == 0 || bn == q.bottleneck ? q.bottleneck : -1;
        }
        if (bn > 0 && bn % 8 == 0 && (net->rm_bn != bn || net->rm_tc0 != net->rs.Tc0 || net->rm_tc != net->rs.Tc)) {
            bridge_gpu_memset(net->rowmask, 0xFF, (size_t)net->rs.Tc * bn / 8);
            bridge_gpu_memset(net->rowmask + (size_t)net->rs.Tc0 * bn / 8, 0, (size_t)bn / 8);
            net->rm_bn = bn;
            net->rm_tc0 = net->rs.Tc0;
            net->rm_tc = net->rs.Tc;
        }
    }
    return repair_vectors();
}

// Self-repair: every site's repair vector in one launch on the chain stream, before the
// first step, from the accumulators as the forward left them (begin() put this stream behind the
// forward's) and the loss scale's device value. The sites' steps add them inside dz's rounding.
bool BackwardPass::repair_vectors() {
    bool any = false;
    for (int li : net->sr_sites) any = any || net->layers[li].sr_act;
    if (!any) return true;
    if (!kf_relu_repair_vectors || !kf_bn_train_bwd_apply_repair || !kf_bn_train_bwd_apply_rows_repair) {
        set_err("backward: this build of libkaldi_fp16 has no self-repair kernels");
        return false;
    }
    return ck(kf_relu_repair_vectors(net->sr_tab.data(), (const KfRepairSite *)net->sr_tab_dev, (int)net->sr_tab.size(),
                                     net->ls_on ? (const float *)net->ls_state : nullptr),
              "self-repair vectors");
}

// The xent branch before the chain walk: ordinary steps seeded with the xent output's gradient,
// on the same rings, events and streams (stepi, flip and nbott advance as for any step, so the
// ring's hazard argument covers them: they are simply the pass's first steps). The last of them
// hands its input gradient to net->gx, gx = rne(acc), which the chain walk's join layer adds:
// g = rne(acc + gx). Both GEMMs run on the chain stream, in order, so the reader is behind the
// writer without an event; the weight-gradient stream never touches gx; and the next
// nnet_backward_xent's writer is behind this call's reader, because finish() joins the chain
// stream into the caller's stream and begin() starts the next pass behind that stream.
bool BackwardPass::branch_pass(const void *xent_grad, const void *out_grad) {
    dz = gcur = xent_grad;
    for (int li : *branch) {
        const int r = step(li, 0);
        if (r == 0) set_err("backward_xent: nothing trainable below " + net->layers[li].L.name);
        if (r != 1) return false;
    }
    dz = gcur = out_grad;
    return true;
}

int BackwardPass::step(int li, int ndone) {
    done = ndone;
    NetLayer &nl = net->layers[li];
    const Layer &L = nl.L;
    // the first compact layer's input gradient: in compact rows with the input layer's
    // mask gathered to them, then scattered to the full rows below (zero elsewhere)
    const bool first_c = net->rs.Tc && li == net->first_c;
    Step s{nl, li, rows_of(net, li), net->T,
           // (the first compact layer read its input gathered to the compact rows)
           first_c && !conv_c_on(net) ? net->xc : act_of(net, nl.input), nl.needs_dx && nl.input >= 0, first_c,
           // (the xent branch's last step: its input gradient goes to gx, not into the ring)
           branch && li == branch->back() ? net->gx : net->dz[flip], net->g[flip],
           // (this step's dbott buffer was last written at step i - 3 or earlier)
           !two ? net->dbott : nbott % 3 == 0 ? net->dbott : nbott % 3 == 1 ? net->dbott2 : net->dbott3, KfEpilogue()};
    if (!side_wait(stepi - 3)) return -1;
    net->dz8_layer[flip] = -1;
    if (s.want_dx && !dx_epilogue(net, nl.input, s.dz_next, s.g_next, s.E, nl.compact)) return -1;
    if (s.want_dx && s.to_full && !to_full_epilogue(s)) return -1;
    if (nl.bypass) {
        s.E.resid = gcur;
        s.E.ldr = L.out_dim;
        s.E.resid_alpha = (float)L.bypass_scale;
    }
    if (branch && li == join_li) {
        // the branch point is a linear-component: it has no bypass, so its producer's residual
        // slot is free
        if (!s.want_dx || s.E.resid || s.E.out || !s.E.out2) {
            set_err("backward_xent: the input gradient of " + L.name + " cannot take the xent branch's gradient");
            return -1;
        }
        s.E.resid = net->gx;
        s.E.ldr = branch_dim;
        s.E.resid_alpha = 1.f;
    }
    bool ok = true;
    switch (L.type) {
        case LayerType::Output:
        case LayerType::Linear: ok = linear(s); break;
        case LayerType::Attention: ok = attention(s); break;
        case LayerType::Prefinal: ok = prefinal(s); break;
        case LayerType::TDNNF: ok = tdnnf(s); break;
        case LayerType::ConvReluBN: ok = conv(s); break;
        case LayerType::CombineFeatureMaps: ok = combine(s); break;
        case LayerType::Batchnorm:
            if (s.want_dx)  // dz already is the gradient at the BN input (dx_epilogue): the same
                            // dz / gcur buffers for the layer below, no flip
                return !net->dp || wgrad([&] { return dp_issue(net, dp_next, done); }) ? 1 : -1;
            break;
        case LayerType::IDCT:
        case LayerType::SpecAugment:
            if (s.want_dx) {
                set_err("backward through " + L.name + " into trainable layers is not supported");
                return -1;
            }
            break;
        default:
            set_err("backward: unsupported layer " + L.name);
            return -1;
    }
    if (!ok || (s.want_dx && s.to_full && !to_full_scatter(s))) return -1;
    // gradient buckets complete at this step go to the communication stream (their
    // gates on side, behind the step's weight gradients)
    if (two) kf_set_stream(net->wg_stream);
    if (net->dp && !dp_issue(net, dp_next, done)) return -1;
    if (two && kf_event_record(net->ev_step[stepi % 3], net->wg_stream) != 0) {
        set_err("backward: weight-gradient stream event");
        return -1;
    }
    to_main();
    if (!s.want_dx) return 0;  // nothing trainable below
    dz = s.dz_next;
    gcur = s.g_next;
    net->dz_last = s.dz_next;
    ++stepi;
    flip = stepi % 3;
    return 1;
}

// the rest of the buckets, then main waits for side (SGD reads every gradient) and for
// every bucket
bool BackwardPass::finish() {
    if (two) kf_set_stream(net->wg_stream);
    if (net->dp && !dp_issue(net, dp_next, INT_MAX)) return false;
    to_main();
    if (!join_side()) return false;
    if (hp) {  // the caller's stream continues after the chain (which joined side)
        if (kf_event_record(net->ev_go, mainst) != 0 || kf_stream_wait(caller, net->ev_go) != 0) {
            set_err("backward: chain stream join");
            return false;
        }
        mainst = caller;
        kf_set_stream(caller);
    }
    if (net->dp && kf_dp_join(net->dp) != 0) {
        set_err(std::string("dp join: ") + (kf_dp_last_error() ? kf_dp_last_error() : ""));
        return false;
    }
    return ng_finish();
}

// the first compact layer's input gradient goes to the compact rows (net->dzc), through the
// input layer's mask gathered to them
bool BackwardPass::to_full_epilogue(Step &s) {
    KfEpilogue &E = s.E;
    const NetLayer &pl = net->layers[s.nl.input];
    const int w = pl.L.out_dim;
    if (E.out || !E.out2 || E.edge_out || E.out8 || (E.mask_in && !pl.mask) || (w * 2) % 16 || (w / 8) % 16) {
        set_err("row subsampling: unsupported input gradient into " + pl.L.name);
        return false;
    }
    if (E.mask_in && !conv_c_on(net)) {  // (a compact conv's mask already is in compact rows)
        if (!ck(kf_gather_rows(net->mc, pl.mask, w / 8, s.Tfull, net->rs.Tc0, net->rs.Tc), "row set mask gather")) return false;
        E.mask_in = net->mc;
    }
    E.out2 = net->dzc;
    return true;
}
bool BackwardPass::to_full_scatter(Step &s) {
    const NetLayer &pl = net->layers[s.nl.input];
    const int w = pl.L.out_dim;
    // (a conv under training-mode BatchNorm took the raw g, dx_epilogue: it belongs in the g slot,
    // where BackwardPass::conv's bn_site_dz reads it and writes dz into the slot left unwritten)
    if (!conv_c_on(net))
        return ck(kf_scatter_rows(pl.bnt_act ? s.g_next : s.dz_next, net->dzc, (long long)w * 2, s.Tfull, net->rs.Tc0,
                                  net->rs.Tc),
                  "row set scatter");
    // the conv below reads the compact rows (net->dzc); only its tail window (full rows
    // from window_t0, conv_window) takes the scattered form
    const int r0 = net->rs.window_t0;
    return net->rs.nt == 0 || ck(kf_scatter_rows_from((char *)s.dz_next + (size_t)r0 * w * 2, net->dzc, (long long)w * 2,
                                                      s.Tfull, net->rs.Tc0, net->rs.Tc, r0),
                                 "row set scatter (tail window)");
}

bool BackwardPass::linear(Step &s) {
    NetLayer &nl = s.nl;
    const int T = s.T, din = nl.L.in_dim, dout = nl.L.out_dim;
    KfOperand A = op_base(s.x, din, T, din, 0);
    KfOperand B = op_base(dz, dout, T, dout, 0);
    if (!wgrad([&] {
            return ck(kf_gemm_wgrad(din, dout, T, &A, &B, gptr(net, nl.pW), dout, gptr(net, nl.pb), 0), "wgrad") &&
                   ng_stats(nl.pW, A, B, T);
        }))
        return false;
    if (!s.want_dx) return true;
    KfOperand A2 = op_base(dz, dout, T, dout, 1);
    KfOperand B2 = op_base(wptr(net, nl.pW), dout, din, dout, 1);
    return dx_wait() && ck(kf_gemm_fused(T, din, dout, &A2, &B2, &s.E), "dgrad");
}

// dz = gradient at the attention output (pre-ReLU, from dx_epilogue); exact attention
// backward into d(affine output), then the affine's weight / bias / input gradients
bool BackwardPass::attention(Step &s) {
    NetLayer &nl = s.nl;
    const int T = s.T, din = nl.L.in_dim, A = att_affine(nl.L);
    KfAttention att = att_args(nl, T);
    if (!ck(kf_attention_backward(&att, dz, nl.L.out_dim, nl.dproj, nl.att_scratch), "attention backward")) return false;
    KfOperand Aw = op_base(s.x, din, T, din, 0);
    KfOperand Bw = op_base(nl.dproj, A, T, A, 0);
    if (!wgrad([&] {
            return ck(kf_gemm_wgrad(din, A, T, &Aw, &Bw, gptr(net, nl.pW), A, gptr(net, nl.pb), 0), "attention wgrad");
        }))
        return false;
    if (!s.want_dx) return true;
    KfOperand A2 = op_base(nl.dproj, A, T, A, 1);
    KfOperand B2 = op_base(wptr(net, nl.pW), A, din, A, 1);
    return dx_wait() && ck(kf_gemm_fused(T, din, A, &A2, &B2, &s.E), "attention dgrad");
}

// dz = gradient at the small (BN2) pre-activation
bool BackwardPass::prefinal(Step &s) {
    NetLayer &nl = s.nl;
    const int T = s.T, din = nl.L.in_dim, big = nl.L.big_dim, small = nl.L.small_dim;
    // training-mode BatchNorm: the layer above left the raw g; BatchNorm 1 has no
    // ReLU below it, so its dz takes no mask
    const bool bnt = nl.bnt_act;
    if (bnt && nl.has_bn2) {
        void *slot = bn_site_slot(nl);
        if (!slot || !bn_site_dz(gcur, nl.bnt_r2, T, bnt_stat_rows(net, s.li), 1, small, nl.bnt_stat2, nl.bn2_rms, nullptr, slot,
                                 "prefinal " + nl.L.name + " (small)"))
            return false;
    }
    KfOperand A = op_base(nl.aux, big, T, big, 0);
    KfOperand B = op_base(dz, small, T, small, 0);
    if (!wgrad([&] {
            return ck(kf_gemm_wgrad(big, small, T, &A, &B, gptr(net, nl.pW2), small, nullptr, 0), "prefinal small wgrad") &&
                   ng_stats(nl.pW2, A, B, T);
        }))
        return false;
    void *dzbig = s.dbott_buf;
    net->dbott_last = dzbig;
    ++nbott;
    KfEpilogue E1 = epi0();
    E1.out2 = dzbig;
    E1.ldo2 = big;
    E1.scale2 = nl.bn_scale;
    E1.mask_in = nl.mask;
    // training mode: the raw gradient at aux into this step's g slot (nothing else is in it until
    // the step's last GEMM, on this stream; the ring's wait for its earlier readers comes first),
    // then BatchNorm 0's backward through the ReLU mask into dzbig
    void *const gbig = s.g_next;
    if (bnt) {
        if (!dx_wait()) return false;
        E1.out2 = gbig;
        E1.scale2 = nullptr;
        E1.mask_in = nullptr;
    }
    KfOperand A1 = op_base(dz, small, T, small, 1);
    KfOperand B1 = op_base(wptr(net, nl.pW2), small, big, small, 1);
    if (!ck(kf_gemm_fused(T, big, small, &A1, &B1, &E1), "prefinal small dgrad")) return false;
    if (bnt && !bn_site_dz(gbig, nl.bnt_r, T, bnt_stat_rows(net, s.li), 1, big, nl.bnt_stat, nl.bn_rms, nl.mask, dzbig,
                           "prefinal " + nl.L.name + " (big)", nl.sr_act ? nl.sr_s : nullptr))
        return false;
    KfOperand A3 = op_base(s.x, din, T, din, 0);
    KfOperand B3 = op_base(dzbig, big, T, big, 0);
    if (!wgrad([&] {
            return ck(kf_gemm_wgrad(din, big, T, &A3, &B3, gptr(net, nl.pW), big, gptr(net, nl.pb), 0), "prefinal big wgrad") &&
                   ng_stats(nl.pW, A3, B3, T);
        }))
        return false;
    if (!s.want_dx) return true;
    KfOperand A4 = op_base(dzbig, big, T, big, 1);
    KfOperand B4 = op_base(wptr(net, nl.pW), big, din, big, 1);
    return dx_wait() && ck(kf_gemm_fused(T, din, big, &A4, &B4, &s.E), "prefinal big dgrad");
}

bool BackwardPass::combine(Step &s) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    if (nl.input2 >= 0 && net->layers[nl.input2].needs_dx + is_trainable(net->layers[nl.input2].L.type)) {
        // the ivector branch: sum the broadcast columns per sequence, then back
        // through its batchnorm-component(s) and linear-component (B rows)
        if (!net->layers[nl.input2].per_seq) {
            set_err("combine " + L.name + ": gradient into a frame-level second input not supported");
            return false;
        }
        const int wb = L.height * L.nf2, rowsB = net->B;
        if (!ck(kf_combine_feature_maps_backward(dz, L.out_dim, net->seq_off, rowsB, nl.gdb, wb, L.height, L.nf1, L.nf2),
                "combine backward"))
            return false;
        const void *gq = nl.gdb;  // the per-sequence gradient on its way down the branch
        for (int cur = nl.input2; cur >= 0; cur = net->layers[cur].input) {
            NetLayer &q = net->layers[cur];
            const int qd = q.L.out_dim;
            if (q.L.type == LayerType::Batchnorm && q.bnt_act) {
                // training-mode BatchNorm over the B rows: its dz into the layer's own
                // buffer (the apply may not write over g)
                if (!bn_site_dz(gq, act_of(net, q.input), rowsB, rowsB, 1, qd, q.bnt_stat, q.bn_rms, nullptr, q.bnt_r,
                                "batchnorm-component " + q.L.name))
                    return false;
                gq = q.bnt_r;
            } else if (q.L.type == LayerType::Batchnorm) {
                if (!ck(kf_scale_cols(gq, qd, q.bn_scale, nl.gdb, qd, rowsB, qd), "ivector bn backward")) return false;
                gq = nl.gdb;
            } else if (q.L.type == LayerType::Linear) {
                if (!wgrad([&] {
                        return ck(kf_rows_wgrad(act_of(net, q.input), q.L.in_dim, gq, qd, gptr(net, q.pW), qd, rowsB,
                                                q.L.in_dim, qd),
                                  "ivector linear wgrad");
                    }))
                    return false;
                if (q.input >= 0) {
                    set_err("ivector branch: a linear-component below another one is not supported");
                    return false;
                }
            } else {
                set_err("ivector branch: unsupported layer " + q.L.name);
                return false;
            }
        }
    }
    if (nl.needs_dx && nl.input >= 0 && net->layers[nl.input].needs_dx + is_trainable(net->layers[nl.input].L.type)) {
        set_err("backward through " + L.name + " into a trainable frame-level input is not supported");
        return false;
    }
    s.want_dx = false;
    return true;
}

// ---------------------------------------------------------------------------
// TDNN-F
// ---------------------------------------------------------------------------
bool BackwardPass::tdnnf(Step &s) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    const int st = nl.compact && net->rs.Tc ? L.time_stride / 3 : L.time_stride, np = st > 0 ? 2 : 1;
    const int ib = dz_index(net, dz);
    const bool imp = ib >= 0 && net->dz_imp[ib];
    // training-mode BatchNorm: the layer above left the raw g (dx_epilogue); a, b over
    // the layer's rows, then dz into the ring buffer its epilogue left unwritten, on the chain
    // stream. Every consumer below, the weight-gradient stream's included (wgrad() orders it
    // behind what the chain enqueued), reads dz as from a frozen layer.
    if (nl.bnt_act && !bn_train_dz(s, ib)) return false;
    Tdnnf t{st, L.bottleneck, np * L.in_dim, np * L.bottleneck, ib, imp, imp ? gcur : dz, nullptr, nullptr};
    // The affine weight gradients run on the weight-gradient stream. (r5, with a
    // two-deep gradient ring, every other one ran on the chain: the chain waited for
    // the side stream before each linear input gradient, and that balanced the two,
    // 36.66 / 36.89 -> 36.55 / 36.65 ms. With the three-deep ring, all on side: 24.81 /
    // 24.89 against 24.96 / 25.13 ms every other, 25.51 / 25.69 all on the chain.)
    // nnet_debug_backward: 1 = every other on the chain, 2 = all on the chain (tests).
    const bool aff_on_main = two && (net->main_aff == 2 || (net->main_aff == 1 && (done & 1)));
    if (!aff_on_main && !wgrad([&] { return tdnnf_affine_wgrad(s, t); })) return false;
    t.w2 = wptr(net, nl.pW2);
    if (t.imp) {
        if (!ck(kf_scale_cols(t.w2, L.out_dim, nl.bn_scale, net->w2s, L.out_dim, t.kaff, L.out_dim), "tdnnf scaled W2"))
            return false;
        t.w2 = net->w2s;
    }
    t.dbott = s.dbott_buf;
    net->dbott_last = t.dbott;
    ++nbott;
    if (!tdnnf_affine_dgrad(s, t) || (aff_on_main && !tdnnf_affine_wgrad(s, t))) return false;
    if (!wgrad([&] { return tdnnf_linear_wgrad(s, t); })) return false;
    return !s.want_dx || (dx_wait() && tdnnf_linear_dgrad(s, t));
}

bool BackwardPass::bn_train_dz(Step &s, int ib) {
    NetLayer &nl = s.nl;
    const int T = s.T, D = nl.L.out_dim;
    if (ib < 0 || gcur == dz || D > net->bnt_w || !kf_bn_train_bwd_stats || !kf_bn_train_bwd_apply) {
        set_err("backward: training-mode BatchNorm of " + nl.L.name + " got no stored output gradient");
        return false;
    }
    const float *sc = nl.bnt_stat + 2 * D, *sh = nl.bnt_stat + 3 * D;
    const float *drop = nl.drop_act ? nl.drop : nullptr;
    const int32_t *rseg = drop ? drop_rows(net, nl.compact) : nullptr;
    float *a = net->bnt_ab, *b = net->bnt_ab + net->bnt_w;
    // compact rows: the statistics were those of the rows c < Tc0, so the sums run over
    // all Tc rows with the divisor Tc0 and only those rows take the correction
    const int Ts = bnt_stat_rows(net, s.li);
    // self-repair: the site's term inside the apply's rounding, on the statistics rows
    const float *repair = nl.sr_act ? nl.sr_s : nullptr;
    if (Ts < T) {
        if (!bn_rows_entries()) return false;
        if (!ck(kf_bn_train_bwd_stats_rows(gcur, D, nl.bnt_r, D, T, Ts, D, sc, sh, nl.bn_rms, drop, D, rseg, a, b),
                "tdnnf batchnorm backward statistics"))
            return false;
        return ck(repair ? kf_bn_train_bwd_apply_rows_repair(gcur, D, nl.bnt_r, D, T, Ts, D, sc, sh, nl.bn_rms, a, b, drop, D, rseg,
                                                             nl.mask, D, net->dz[ib], D, repair)
                         : kf_bn_train_bwd_apply_rows(gcur, D, nl.bnt_r, D, T, Ts, D, sc, sh, nl.bn_rms, a, b, drop, D, rseg,
                                                      nl.mask, D, net->dz[ib], D),
                  "tdnnf batchnorm backward apply");
    }
    if (!ck(kf_bn_train_bwd_stats(gcur, D, nl.bnt_r, D, T, D, sc, sh, nl.bn_rms, drop, D, rseg, a, b),
            "tdnnf batchnorm backward statistics"))
        return false;
    return ck(repair ? kf_bn_train_bwd_apply_repair(gcur, D, nl.bnt_r, D, T, D, sc, sh, nl.bn_rms, a, b, drop, D, rseg, nl.mask, D,
                                                    net->dz[ib], D, repair)
                     : kf_bn_train_bwd_apply(gcur, D, nl.bnt_r, D, T, D, sc, sh, nl.bn_rms, a, b, drop, D, rseg, nl.mask, D,
                                             net->dz[ib], D),
              "tdnnf batchnorm backward apply");
}
// the _rows entries a backward on compact rows needs (weak references, net_internal.h)
bool BackwardPass::bn_rows_entries() {
    if (kf_bn_train_bwd_stats_rows && kf_bn_train_bwd_apply_rows) return true;
    set_err("backward: this build of libkaldi_fp16 has no training-mode BatchNorm kernels for the row-subsampled step");
    return false;
}

// Training-mode BatchNorm backward of a conv, prefinal or batchnorm-component site:
// a, b over g and r [rows x H F] (block f = column h F + f), then dz = scale (g - a - yhat b)
// relu_bit through the dense [rows H x F] view, on the chain stream. mask NULL: no ReLU below the
// BatchNorm. One a | b pair serves every site: the chain stream runs them in order. stat_rows < rows:
// the statistics were those of the first stat_rows rows (the _rows entries).
bool BackwardPass::bn_site_dz(const void *g, const void *r, int rows, int stat_rows, int H, int F, const float *stat, float rms,
                              const uint8_t *mask, void *dz_out, const std::string &what, const float *repair) {
    if (!g || !r || !stat || !dz_out || g == dz_out || F > net->bnt_w || !kf_bn_train_bwd_stats || !kf_bn_train_bwd_apply ||
        (H > 1 && !kf_bn_block_bwd_stats)) {
        set_err("backward: training-mode BatchNorm of " + what + " got no stored output gradient");
        return false;
    }
    const float *sc = stat + 2 * F, *sh = stat + 3 * F;
    float *a = net->bnt_ab, *b = net->bnt_ab + net->bnt_w;
    if (stat_rows < rows) {  // a prefinal layer on compact rows (H = 1: no conv is compact under the mode)
        if (H != 1) set_err("backward: training-mode BatchNorm of " + what + " has block statistics on a row subset");
        if (H != 1 || !bn_rows_entries()) return false;
        return ck(kf_bn_train_bwd_stats_rows(g, F, r, F, rows, stat_rows, F, sc, sh, rms, nullptr, 0, nullptr, a, b),
                  (what + " batchnorm backward statistics").c_str()) &&
               ck(repair ? kf_bn_train_bwd_apply_rows_repair(g, F, r, F, rows, stat_rows, F, sc, sh, rms, a, b, nullptr, 0, nullptr,
                                                             mask, F, dz_out, F, repair)
                         : kf_bn_train_bwd_apply_rows(g, F, r, F, rows, stat_rows, F, sc, sh, rms, a, b, nullptr, 0, nullptr, mask,
                                                      F, dz_out, F),
                  (what + " batchnorm backward apply").c_str());
    }
    const int rc = H == 1 ? kf_bn_train_bwd_stats(g, F, r, F, rows, F, sc, sh, rms, nullptr, 0, nullptr, a, b)
                          : kf_bn_block_bwd_stats(g, (long long)H * F, r, (long long)H * F, rows, H, F, sc, sh, rms, a, b);
    return ck(rc, (what + " batchnorm backward statistics").c_str()) &&
           ck(repair ? kf_bn_train_bwd_apply_repair(g, F, r, F, rows * H, F, sc, sh, rms, a, b, nullptr, 0, nullptr, mask, F, dz_out,
                                                    F, repair)
                     : kf_bn_train_bwd_apply(g, F, r, F, rows * H, F, sc, sh, rms, a, b, nullptr, 0, nullptr, mask, F, dz_out, F),
              (what + " batchnorm backward apply").c_str());
}
// the ring slot a governed layer's dz goes to: the one its producer's epilogue left unwritten
// (dx_epilogue stored the raw g beside it), or NULL when the step was not seeded that way
void *BackwardPass::bn_site_slot(const NetLayer &nl) {
    const int ib = dz_index(net, dz);
    if (ib >= 0 && gcur != dz) return net->dz[ib];
    set_err("backward: training-mode BatchNorm of " + nl.L.name + " got no stored output gradient");
    return nullptr;
}

KfOperand BackwardPass::masked(const Step &s, const Tdnnf &t, KfOperand o) const {
    if (t.imp) {
        o.mask = s.nl.mask;
        o.mask_rows = s.T;
    }
    return o;
}

// affine weight / bias gradient: splice+(bott)^T . dz
bool BackwardPass::tdnnf_affine_wgrad(Step &s, const Tdnnf &t) {
    NetLayer &nl = s.nl;
    const int T = s.T, dout = nl.L.out_dim;
    KfOperand A = t.s > 0 ? op_splice(nl.aux, T, t.bn, 0, t.s, KF_CLAMP, 0) : op_base(nl.aux, t.bn, T, t.bn, 0);
    KfOperand B = masked(s, t, op_base(t.dzs, dout, T, dout, 0));
    if (t.imp)
        return ck(kf_gemm_wgrad_scaled(t.kaff, dout, T, &A, &B, gptr(net, nl.pW2), dout, gptr(net, nl.pb2), 0, nl.bn_scale),
                  "tdnnf affine wgrad");
    return ck(kf_gemm_wgrad(t.kaff, dout, T, &A, &B, gptr(net, nl.pW2), dout, gptr(net, nl.pb2), 0), "tdnnf affine wgrad") &&
           ng_stats(nl.pW2, A, B, T);
}

// bottleneck gradient: transpose of the [0, +s] clamped splice
bool BackwardPass::tdnnf_affine_dgrad(Step &s, const Tdnnf &t) {
    NetLayer &nl = s.nl;
    const int T = s.T, dout = nl.L.out_dim, bn = t.bn;
    KfEpilogue E1 = epi0();
    E1.out = t.dbott;
    E1.ldo = bn;
    // compact rows with a tail: the scratch row Tc0 read row Tc0 - 1's gradient
    // through the +1 adjacency; its true gradient is zero (written as zero through
    // the row mask)
    bool zero_scratch = nl.compact && net->rs.Tc > net->rs.Tc0 && t.s > 0;
    if (zero_scratch && net->rowmask && net->rm_bn == bn && net->rm_tc0 == net->rs.Tc0 && net->rm_tc == net->rs.Tc) {
        E1.out = nullptr;
        E1.out2 = t.dbott;
        E1.ldo2 = bn;
        E1.mask_in = net->rowmask;
        zero_scratch = false;
    }
    if (t.s == 0) {
        KfOperand A1 = masked(s, t, op_base(t.dzs, dout, T, dout, 1));
        KfOperand B1 = op_base(t.w2, dout, bn, dout, 1);
        return ck(kf_gemm_fused(T, bn, dout, &A1, &B1, &E1), "tdnnf affine dgrad");
    }
    if (s.want_dx) {
        // the linear input gradient's edge row (row T of dbott: sum of rows 0 .. s),
        // summed by this GEMM's first row tile
        E1.edge_out = (char *)t.dbott + (size_t)T * bn * 2;
        E1.edge_r0 = 0;
        E1.edge_r1 = t.s + 1 < T ? t.s + 1 : T;
        E1.edge_src = E1.out2 ? 1 : 0;
    }
    // spare row T of dz (of g when dz is implicit: the masked sum) holds
    // sum_{t >= T-1-s} dz[t] (clamped-splice transpose)
    void *edge = (char *)t.dzs + (size_t)T * dout * 2;
    const bool have_edge = !t.imp && t.ib >= 0 && net->dz_edge[t.ib];  // dx_epilogue's
    if (nl.compact && net->rs.Tc) {
        // compact rows: the source rows T-1-3 .. T-1 that are in the set, in
        // source order (the others carry no gradient)
        int rows[4], nr = 0;
        for (int f = std::max(0, s.Tfull - 1 - nl.L.time_stride); f < s.Tfull; ++f) {
            const int c = net->rs.compact_of(f);
            if (c >= 0 && nr < 4) rows[nr++] = c;
        }
        if (!ck(kf_rows_sum_list(edge, t.dzs, dout, rows, nr, dout), "row set edge")) return false;
    } else if (!have_edge && !ck(kf_rows_sum_mask(edge, t.dzs, dout, T - 1 - t.s < 0 ? 0 : T - 1 - t.s, T, dout,
                                                  t.imp ? nl.mask : nullptr),
                                 "edge"))
        return false;
    if (net->fp8 && t.ib >= 0 && net->dz8_layer[t.ib] == s.li && T > 1) return tdnnf_affine_dgrad_mx(s, t, E1, edge);
    KfOperand A1 = masked(s, t, op_splice(t.dzs, T, dout, 0, -t.s, KF_ZERO, 1));
    A1.edge_t[1] = T - 1;
    A1.edge_row[1] = T;
    KfOperand B1 = op_wrows(t.w2, 2, bn, dout);
    if (!ck(kf_gemm_fused(T, bn, 2 * dout, &A1, &B1, &E1), "tdnnf affine dgrad")) return false;
    if (zero_scratch)  // (no row mask for this bottleneck width)
        bridge_gpu_memset((char *)t.dbott + (size_t)net->rs.Tc0 * bn * 2, 0, (size_t)bn * 2);
    return true;
}

// MXFP8 (the one MFMA-bound backward product, K = 2 x dout): rows 0 .. T-2 from dz's e4m3
// copy [dz(t) | dz(t-s)] against the e4m3 weight rows; row T-1, whose second part is the
// clamped-edge sum, again in fp16 (the MXFP8 operand has no edge rows)
bool BackwardPass::tdnnf_affine_dgrad_mx(Step &s, const Tdnnf &t, const KfEpilogue &E1, void *edge) {
    NetLayer &nl = s.nl;
    const int T = s.T, dout = nl.L.out_dim, bn = t.bn;
    const Mx &d8 = net->dz8[t.ib];
    const int pw = pad128(dout);
    KfOperand A1 = op_base(d8.q, d8.ld, T, 2 * pw, 1);
    A1.nparts = 2;
    A1.part_width = pw;
    A1.dt[1] = -t.s;
    A1.tpolicy = KF_ZERO;
    A1.fmt = KF_FMT_MXFP8;
    A1.scales = d8.s;
    A1.lds = d8.ld / 32;
    KfOperand B8 = op_mxw(nl.w8d, bn);
    // rows 0 .. T-2, and row T-1 by the last row tile's workgroups
    return ck(kf_gemm_fused_edge(T - 1, bn, 2 * pw, &A1, &B8, &E1, (char *)t.dbott + (size_t)(T - 1) * bn * 2,
                                 (const char *)dz + (size_t)(T - 1) * dout * 2, edge, wptr(net, nl.pW2), dout),
              "tdnnf affine dgrad mxfp8");
}

// linear weight gradient: splice-(x)^T . dbott
bool BackwardPass::tdnnf_linear_wgrad(Step &s, const Tdnnf &t) {
    const int T = s.T, din = s.nl.L.in_dim;
    KfOperand A2 = t.s > 0 ? op_splice(s.x, T, din, -t.s, 0, KF_CLAMP, 0) : op_base(s.x, din, T, din, 0);
    KfOperand B2 = op_base(t.dbott, t.bn, T, t.bn, 0);
    return ck(kf_gemm_wgrad(t.klin, t.bn, T, &A2, &B2, gptr(net, s.nl.pW), t.bn, nullptr, 0), "tdnnf linear wgrad") &&
           ng_stats(s.nl.pW, A2, B2, T);
}

// input gradient: transpose of the [-s, 0] clamped splice
bool BackwardPass::tdnnf_linear_dgrad(Step &s, const Tdnnf &t) {
    const int T = s.T, din = s.nl.L.in_dim, bn = t.bn;
    if (t.s > 0) {
        // spare row T of dbott holds sum_{t <= s} dbott[t]
        // (row T of dbott: the affine input gradient's epilogue summed it, E1)
        KfOperand A3 = op_splice(t.dbott, T, bn, t.s, 0, KF_ZERO, 1);
        A3.edge_t[0] = 0;
        A3.edge_row[0] = T;
        KfOperand B3 = op_wrows(wptr(net, s.nl.pW), 2, din, bn);
        return ck(kf_gemm_fused(T, din, 2 * bn, &A3, &B3, &s.E), "tdnnf linear dgrad");
    }
    KfOperand A3 = op_base(t.dbott, bn, T, bn, 1);
    KfOperand B3 = op_base(wptr(net, s.nl.pW), bn, din, bn, 1);
    return ck(kf_gemm_fused(T, din, bn, &A3, &B3, &s.E), "tdnnf linear dgrad");
}

// ---------------------------------------------------------------------------
// conv-relu-batchnorm
// ---------------------------------------------------------------------------
bool BackwardPass::conv(Step &s) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    const bool compact = conv_compact(net, s.li);
    // training-mode BatchNorm: the layer above left the raw g; per filter a, b over
    // rows x height-out, then dz into the ring slot, before anything below reads dz
    if (nl.bnt_act) {
        void *slot = bn_site_slot(nl);
        if (!slot || !bn_site_dz(gcur, nl.bnt_r, s.T, s.T, L.hout, L.fout, nl.bnt_stat, nl.bn_rms, nl.mask, slot, "conv " + L.name,
                                 nl.sr_act ? nl.sr_s : nullptr))
            return false;
    }
    // compact-row conv: the tail window runs first, on the weight-gradient stream beside
    // the residue GEMMs (conv_window)
    if (s.want_dx && compact && net->rs.nt > 0 && two && s.E.out2 && !conv_window(s, true)) return false;
    if (nl.kp) return conv_small_fin(s);
    if (L.fin == 1) {
        if (!wgrad([&] {
                return ck(kf_conv_c1_wgrad(s.T, L.hin, L.hout, L.hsub, L.fout, (int)nl.dt.size(), nl.dt.data(),
                                           nl.dh.data(), s.x, dz, gptr(net, nl.pW), gptr(net, nl.pb)),
                          "conv c1 wgrad");
            }))
            return false;
    } else if (!wgrad([&] { return compact ? conv_wgrad_compact(s) : conv_wgrad_plain(s); })) {
        return false;
    }
    if (!s.want_dx) return true;
    if (!dx_wait()) return false;
    if (L.fin == 1) {
        set_err("conv " + L.name + ": input gradient of a 1-filter conv not supported");
        return false;
    }
    if (compact) return conv_dgrad_compact(s);
    if (L.hsub > 1 && L.hin % L.hsub == 0 && !s.E.out) return conv_dgrad_strided(s);
    return conv_dgrad_plain(s);
}

// small fin: the forward's im2col is still in nl.im2col
bool BackwardPass::conv_small_fin(Step &s) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    const int T = s.T, noff = (int)nl.dt.size(), K = noff * L.fin;
    KfEpilogue &E = s.E;
    // wgrad over the padded K (the pad columns are zero), then the first
    // ntaps*fin rows into the flat gradient
    KfOperand A = op_base(nl.im2col, nl.kp, T * L.hout, nl.kp, 0);
    KfOperand B = op_base(dz, L.fout, T * L.hout, L.fout, 0);
    if (!wgrad([&] {
            return ck(kf_gemm_wgrad(nl.kp, L.fout, T * L.hout, &A, &B, nl.gwpad, L.fout, gptr(net, nl.pb), 0),
                      "conv small-fin wgrad") &&
                   ck(ops_copy(gptr(net, nl.pW), nl.gwpad, 2 * K * L.fout), "conv small-fin wgrad copy");
        }))
        return false;
    if (!s.want_dx) return true;
    // the input gradient overwrites nl.im2col, which the weight gradient
    // just read on side: main waits for side here
    if (!join_side()) return false;
    waited = stepi - 1;
    if (E.out || E.mask_in || E.scale2 || !E.out2) {
        set_err("conv " + L.name + ": small-fin input gradient only into combine-feature-maps");
        return false;
    }
    // dP = dz . Wpad^T into the im2col buffer, then the gather col2im
    KfOperand A2 = op_base(dz, L.fout, T * L.hout, L.fout, 1);
    KfOperand B2 = op_base(nl.wpad, L.fout, nl.kp, L.fout, 1);
    KfEpilogue Ed = epi0();
    Ed.out = nl.im2col;
    Ed.ldo = nl.kp;
    return ck(kf_gemm_fused(T * L.hout, nl.kp, L.fout, &A2, &B2, &Ed), "conv small-fin dgrad") &&
           ck(kf_col2im_small(nl.im2col, T, L.hin, L.hout, L.hsub, L.fin, noff, nl.dt.data(), nl.dh.data(), nl.kp, E.out2,
                              L.in_dim),
              "col2im small");
}

bool BackwardPass::conv_wgrad_plain(Step &s) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    KfOperand A = op_im2col(nl, s.x, s.T, 0);
    KfOperand B = op_base(dz, L.fout, s.T * L.hout, L.fout, 0);
    return ck(kf_gemm_wgrad((int)nl.dt.size() * L.fin, L.fout, s.T * L.hout, &A, &B, gptr(net, nl.pW), L.fout,
                            gptr(net, nl.pb), 0),
              "conv wgrad");
}

// output gradient on the compact rows only (net->dzc): the reduction over
// output frames 3c (c < Tc0), then over the tail frames, added
bool BackwardPass::conv_wgrad_compact(Step &s) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    const RowSet &rs = net->rs;
    const int K = (int)nl.dt.size() * L.fin;
    KfOperand A = op_im2col(nl, s.x, s.T, 0);
    A.tmul = 3;
    A.nrows = rs.Tc0 * L.hout;
    KfOperand B = op_base(net->dzc, L.fout, rs.Tc0 * L.hout, L.fout, 0);
    if (!ck(kf_gemm_wgrad(K, L.fout, rs.Tc0 * L.hout, &A, &B, gptr(net, nl.pW), L.fout, gptr(net, nl.pb), 0),
            "conv wgrad (compact rows)"))
        return false;
    if (rs.nt == 0) return true;
    A.t0 = rs.tail_t0;
    A.nrows = rs.nt * L.hout;
    B.base = (const char *)net->dzc + (size_t)rs.Tc0 * L.hout * L.fout * 2;
    B.nrows = B.T = rs.nt * L.hout;
    return ck(kf_gemm_wgrad(K, L.fout, rs.nt * L.hout, &A, &B, gptr(net, nl.pW), L.fout, gptr(net, nl.pb), 1),
              "conv wgrad (compact tail rows)");
}

// compact-row conv: the input gradient of the frames the tail reaches (window_t0 ...) comes
// from the full-row kernel on a window of the scattered output gradient dz (zero below it).
// side = true: on the weight-gradient stream; main joins it after the residue GEMMs.
bool BackwardPass::conv_window(Step &s, bool side) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    const int noff = (int)nl.dt.size(), w0 = net->rs.window_t0, tw = s.T - w0;
    KfOperand A2 = op_col2im(nl, (const char *)dz + (long long)w0 * L.hout * L.fout * 2, tw);
    KfOperand B2 = op_wrows(wptr(net, nl.pW), noff, L.fin, L.fout);
    KfEpilogue Ew = at_frame(s.E, L, w0);
    auto window = [&] { return ck(kf_gemm_fused(tw * L.hin, L.fin, noff * L.fout, &A2, &B2, &Ew), "conv dgrad (tail window)"); };
    if (!side) return window();
    return to_side() && side_launch(net, mainst, "backward: conv window", window);
}

// The output gradient is non-zero on the compact frames only (net->dzc): input frame
// f = 3c + e receives only the taps with dt = e, from compact frame c. One GEMM per residue
// e over those taps, its rows written to frames 3c + e in place (grouped epilogue rows);
// every nonzero term in the full-row kernel's order, so the result is bit-identical. The
// frames the tail reaches take the full-row kernel (conv_window): on the weight-gradient
// stream it went first, at the start of this step, and main joins it after the residues.
bool BackwardPass::conv_dgrad_compact(Step &s) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    const KfEpilogue &E = s.E;
    const RowSet &rs = net->rs;
    if (!E.out2 || E.out8 || E.edge_out || E.resid || E.beta != 0.f) {
        set_err("row subsampling: unsupported input gradient of " + L.name);
        return false;
    }
    const int noff = (int)nl.dt.size();
    const long long fo = (long long)L.hout * L.fout;
    if (rs.nt > 0 && !two && !conv_window(s, false)) return false;
    for (int e = -1; e <= 1; ++e) {
        const int c_hi = std::min(rs.Tc0, (rs.residue_last_frame - e) / 3 + 1), c_lo = e < 0 ? 1 : 0;
        if (c_hi <= c_lo) continue;
        KfOperand A2 = op_col2im(nl, (const char *)net->dzc + c_lo * fo * 2, c_hi - c_lo);
        KfOperand B2 = op_wrows(wptr(net, nl.pW), noff, L.fin, L.fout);
        int np = 0;
        for (int o = 0; o < noff; ++o) {
            if (nl.dt[o] != e) continue;
            A2.dt[np] = 0;
            A2.dh[np] = -nl.dh[o];
            B2.dt[np] = o * L.fin;
            ++np;
        }
        A2.nparts = B2.nparts = np;
        A2.ncols = B2.ncols = np * L.fout;
        KfEpilogue Er = at_frame(E, L, 3LL * c_lo + e);
        Er.row_group = L.hin;
        Er.row_stride = 3 * L.hin;
        if (!ck(kf_gemm_fused((c_hi - c_lo) * L.hin, L.fin, np * L.fout, &A2, &B2, &Er), "conv dgrad (compact rows)"))
            return false;
    }
    return !(rs.nt > 0 && two) || aux_join(net, mainst, "backward: conv window");
}

// strided conv: input row h' = hsub*j + pi only receives the taps with (pi - dh) % hsub == 0,
// so one GEMM per residue pi skips the (hsub-1)/hsub of the K range the plain col2im reads
// as zeros
bool BackwardPass::conv_dgrad_strided(Step &s) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    const KfEpilogue &E = s.E;
    const int T = s.T, noff = (int)nl.dt.size(), hs = L.hsub;
    // every residue's taps, residue by residue: pi's are taps[first[pi] .. first[pi + 1])
    std::vector<int> taps, first(hs + 1, 0);
    for (int pi = 0; pi < hs; ++pi) {
        for (int o = 0; o < noff; ++o)
            if (!((((pi - nl.dh[o]) % hs) + hs) % hs)) taps.push_back(o);
        first[pi + 1] = (int)taps.size();
    }
    const bool twt = dgrad_wt_on();
    char *wt = nullptr;
    if (twt && !(wt = (char *)dgrad_wt(net, nl, taps))) {
        set_err("conv dgrad (strided): transposed weights of " + L.name);
        return false;
    }
    for (int pi = 0; pi < hs; ++pi) {
        const int np = first[pi + 1] - first[pi];
        if (!np) continue;
        KfOperand A2 = op_col2im(nl, dz, T);
        KfOperand B2 = op_wrows(wptr(net, nl.pW), noff, L.fin, L.fout);
        for (int i = 0; i < np; ++i) {
            const int o = taps[first[pi] + i];
            A2.dt[i] = -nl.dt[o];
            A2.dh[i] = (pi - nl.dh[o]) / hs;  // exact: a multiple of hsub
            B2.dt[i] = o * L.fin;
        }
        A2.nparts = B2.nparts = np;
        A2.ncols = B2.ncols = np * L.fout;
        if (twt) B2 = op_base(wt + (size_t)first[pi] * L.fin * L.fout * 2, L.fin, np * L.fout, L.fin, 0);
        A2.hout = L.hin / hs;
        A2.hmul = 1;
        A2.hdiv = 1;
        A2.nrows = T * A2.hout;
        KfEpilogue Ep = E;  // rows hsub*m + pi of the [(t,h) x fin] gradient
        Ep.out2 = (char *)E.out2 + (size_t)pi * L.fin * 2;
        Ep.ldo2 = (long long)hs * L.fin;
        if (E.mask_in) Ep.mask_in = E.mask_in + (size_t)pi * L.fin / 8;
        if (!ck(kf_gemm_fused(T * A2.hout, L.fin, np * L.fout, &A2, &B2, &Ep), "conv dgrad (strided)")) return false;
    }
    return true;
}

bool BackwardPass::conv_dgrad_plain(Step &s) {
    NetLayer &nl = s.nl;
    const Layer &L = nl.L;
    KfEpilogue &E = s.E;
    const int noff = (int)nl.dt.size();
    KfOperand A2 = op_col2im(nl, dz, s.T);
    KfOperand B2 = op_wrows(wptr(net, nl.pW), noff, L.fin, L.fout);
    if (dgrad_wt_on()) {
        std::vector<int> taps(noff);
        for (int o = 0; o < noff; ++o) taps[o] = o;
        void *wt = dgrad_wt(net, nl, taps);
        if (!wt) {
            set_err("conv dgrad: transposed weights of " + L.name);
            return false;
        }
        B2 = op_base(wt, L.fin, noff * L.fout, L.fin, 0);
    }
    E.ldo2 = L.fin;  // dz of the input conv layer viewed as [(t,h) x fin]
    if (E.out) E.ldo = L.fin;
    return ck(kf_gemm_fused(s.T * L.hin, L.fin, noff * L.fout, &A2, &B2, &E), "conv dgrad");
}

// xent_grad != NULL: `branch` holds the xent branch's layers, `join` the chain-path layer that
// reads the branch point (nnet_backward_xent)
int backward_impl(KfNet *net, const void *out_grad, int max_layers, const void *xent_grad = nullptr,
                  const std::vector<int> *branch = nullptr, int join = -1) {
    if (!on_device(net, "backward")) return -1;
    if (net->T <= 0) {
        set_err("backward before forward");
        return -1;
    }
    BackwardPass pass(net, out_grad);
    if (xent_grad) {
        pass.branch = branch;
        pass.join_li = join;
        pass.branch_dim = net->layers[net->layers[join].input].L.out_dim;
    }
    if (!pass.begin()) return -1;
    if (xent_grad && !pass.branch_pass(xent_grad, out_grad)) return -1;
    for (int li = net->chain_out, done = 0; li >= 0 && done < max_layers; li = net->layers[li].input, ++done) {
        const int r = pass.step(li, done);
        if (r < 0) return -1;
        if (r == 0) break;
    }
    return pass.finish() ? 0 : -1;
}

}  // namespace

extern "C" int nnet_backward(KfNet *net, const void *out_grad) {
    kf_take_pending(__func__);
    return backward_impl(net, out_grad, 1 << 30);
}
// Two seeds: the chain output's gradient and, at the log-softmax output named
// output-xent, the xent gradient of kf_chain_xent, both in the forward's row form.
extern "C" int nnet_backward_xent(KfNet *net, const void *out_grad, const void *xent_grad) {
    kf_take_pending(__func__);
    if (!on_device(net, "backward_xent")) return -1;
    if (!out_grad || !xent_grad) {
        set_err("backward_xent: null gradient");
        return -1;
    }
    int xo = -1;
    for (size_t i = 0; i < net->layers.size(); ++i)
        if (net->layers[i].L.type == LayerType::Output && net->layers[i].L.name == "output-xent") xo = (int)i;
    if (xo < 0 || xo == net->chain_out) {
        set_err("backward_xent: the network has no output-xent layer beside the chain output");
        return -1;
    }
    std::vector<char> on(net->layers.size(), 0);
    for (int cur = net->chain_out; cur >= 0; cur = net->layers[cur].input) on[cur] = 1;
    std::vector<int> branch;
    int bp = xo;
    for (; bp >= 0 && !on[bp]; bp = net->layers[bp].input) branch.push_back(bp);
    if (bp < 0) {
        set_err("backward_xent: the path from output-xent down does not reach the chain output's path");
        return -1;
    }
    if (net->layers[bp].L.type != LayerType::Linear) {
        set_err("backward_xent: the branch point " + net->layers[bp].L.name + " is not a linear-component");
        return -1;
    }
    int join = -1;
    for (int cur = net->chain_out; cur >= 0; cur = net->layers[cur].input)
        if (net->layers[cur].input == bp) join = cur;
    if (join < 0 || net->layers[join].bypass) {
        set_err("backward_xent: no chain-path layer without a bypass reads the branch point " + net->layers[bp].L.name);
        return -1;
    }
    if (!admit(net, Mode::XentBackward, "backward_xent")) return -1;
    if (!net->gx) {  // the branch's gradient at the branch point, fp16 [max_T x dim]: made once
        net->gx = net->dalloc((size_t)net->max_T * net->layers[bp].L.out_dim * 2);
        if (!net->gx) {
            set_err("backward_xent: alloc the branch gradient");
            return -1;
        }
    }
    return backward_impl(net, out_grad, 1 << 30, xent_grad, &branch, join);
}
// debugging / tests: back-propagate through the top `n` layers only
extern "C" int nnet_backward_n(KfNet *net, const void *out_grad, int n) {
    if (net && !admit(net, Mode::BackwardN, "backward_n")) return -1;
    return backward_impl(net, out_grad, n);
}
// debugging / tests: device pointers of internal tensors
extern "C" const void *nnet_debug_tensor(KfNet *net, const char *what, int layer) {
    std::string w = what;
    if (w == "dzlast") return net->dz_last;
    for (int i = 0; i < 3; ++i) {
        if (w == "dz" + std::to_string(i)) return net->dz[i];
        if (w == "g" + std::to_string(i)) return net->g[i];
    }
    if (w == "dbott") return net->dbott_last ? net->dbott_last : net->dbott;
    if (w == "vel") return net->vel;  // the updates' velocity, fp32 [num_params]
    // the MXFP8 copies of dz[layer] (layer = buffer 0 / 1) and the layer whose affine input
    // gradient reads it (as an int, through the pointer's low bits: -1 none), MXFP8 train step
    if ((w == "dz8q" || w == "dz8s" || w == "dz8layer") && layer >= 0 && layer <= 2) {
        if (w == "dz8layer") return (const void *)(intptr_t)(net->dz8_layer[layer] + 1);
        return w == "dz8q" ? (const void *)net->dz8[layer].q : (const void *)net->dz8[layer].s;
    }
    if (layer < 0 || layer >= (int)net->layers.size()) return nullptr;
    if (w == "aux") return net->layers[layer].aux;
    if (w == "dproj") return net->layers[layer].dproj;
    if (w == "gdb") return net->layers[layer].gdb;
    if (w == "mask") return net->layers[layer].mask;
    if (w == "bn_scale") return net->layers[layer].bn_scale;
    if (w == "bn2_scale") return net->layers[layer].bn2_scale;
    if (w == "bn_shift") return net->layers[layer].bn_shift;
    if (w == "bn2_shift") return net->layers[layer].bn2_shift;
    // the e4m3 affine weight rows of the MXFP8 input gradient, [bn x 2*pad128(out)]
    if (w == "w8dq") return net->layers[layer].w8d.q;
    if (w == "w8ds") return net->layers[layer].w8d.s;
    // the MXFP8 copy this layer's GEMM reads (e4m3 [T x pad128(in)], E8M0 [T x pad128(in)/32])
    if (w == "x8q" || w == "x8s") {
        const Mx *m = in8(net, net->layers[layer]);
        return !m ? nullptr : w == "x8q" ? (const void *)m->q : (const void *)m->s;
    }
    return nullptr;
}
