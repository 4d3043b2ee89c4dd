// natgrad.cpp — natural-gradient preconditioning: nnet_set_natural_gradient and its getters.
#include "net_internal.h"

// ---------------------------------------------------------------------------
// Natural-gradient preconditioning (kf_nnet.h nnet_set_natural_gradient): the
// tables and buffers; nnet_backward (backward.cpp) issues the statistics and the launches
// ---------------------------------------------------------------------------
static int ng_rp(int R) { return (R + 31) / 32 * 32; }

// a side's rank: at most half its dimension (and what the state kernel holds); below 8 the
// side is left unpreconditioned (0)
static int ng_rank(int want, int dim) {
    const int r = std::min(std::min(want, dim / 2), (int)KF_NG_MAX_RANK);
    return r >= 8 ? r : 0;
}

extern "C" int nnet_set_natural_gradient(KfNet *net, const KfNgOpts *opts) {
    kf_take_pending(__func__);
    if (!on_device(net, "set_natural_gradient")) return -1;
    if (!opts) {
        net->ng_on = false;
        return 0;
    }
    if (!kf_ng_init || !kf_ng_apply_scratch_bytes || !kf_ng_state_scratch_bytes) {
        set_err("set_natural_gradient: this build of libkaldi_fp16 has no kf_ng_* kernels");
        return -1;
    }
    if (!admit(net, Mode::NaturalGradient, "set_natural_gradient")) return -1;
    if (opts->rank_in < 0 || opts->rank_out < 0 || opts->update_period < 1 || !(opts->num_samples_history > 0.f) ||
        !(opts->alpha >= 0.f) || !(opts->epsilon > 0.f) || !(opts->delta >= 0.f)) {
        set_err("set_natural_gradient: bad options");
        return -1;
    }
    net->ng_on = false;
    net->ng_opts = *opts;
    net->ng_pres.clear();
    net->ng_comps.clear();
    net->ng_pre_comp.clear();
    net->ng_pre_side.clear();
    net->ng_of_param.assign(net->params.size(), -1);
    auto off_path = [&](long long off) {
        for (const auto &r : net->offpath)
            if (off >= r.first && off < r.first + r.second) return true;
        return false;
    };
    long long w = 0, h = 0, s = 0, st = 0;
    auto add_pre = [&](int D, int R, int comp, int side) {
        const int Rp = ng_rp(R);
        net->ng_pres.push_back(KfNgPre{D, R, w, h, s, st});
        net->ng_pre_comp.push_back(comp);
        net->ng_pre_side.push_back(side);
        w += (long long)Rp * D;
        h += KF_NG_W16_HALFS(D, Rp);
        s += 2 + Rp;
        st += KF_NG_STAT_FLOATS(D, Rp);
        return (int)net->ng_pres.size() - 1;
    };
    // the update component of a weight tensor and its bias
    auto add_comp = [&](int pW, int pb) {
        if (pW < 0) return;
        const ParamRef &p = net->params[pW];
        if (off_path(p.off)) return;  // no gradient: nnet_backward zeroes it
        int ci = -1;
        for (size_t c = 0; c < net->comps.size(); ++c)
            if (pW >= net->comps[c].first && pW < net->comps[c].first + net->comps[c].count) ci = (int)c;
        const int din = p.rows + (pb >= 0 ? 1 : 0);
        const int rin = ng_rank(opts->rank_in, din), rout = ng_rank(opts->rank_out, p.cols);
        if (!rin && !rout) return;
        KfNgComp c{p.off, pb >= 0 ? net->params[pb].off : -1, p.rows, p.cols, -1, -1};
        if (rin) c.pre_in = add_pre(din, rin, ci, 0);
        if (rout) c.pre_out = add_pre(p.cols, rout, ci, 1);
        net->ng_of_param[pW] = (int)net->ng_comps.size();
        net->ng_comps.push_back(c);
    };
    int max_rp = 0;
    for (const NetLayer &nl : net->layers) {
        const LayerType t = nl.L.type;
        if (nl.per_seq) continue;
        if (t == LayerType::Linear || t == LayerType::Output) add_comp(nl.pW, nl.pb);
        if (t == LayerType::TDNNF || t == LayerType::Prefinal) {
            add_comp(nl.pW, t == LayerType::Prefinal ? nl.pb : -1);
            add_comp(nl.pW2, t == LayerType::TDNNF ? nl.pb2 : -1);
        }
    }
    for (const KfNgPre &p : net->ng_pres) max_rp = std::max(max_rp, ng_rp(p.R));
    net->ng_issued.assign(net->ng_comps.size(), 0);
    net->ng_t = 0;
    net->ng_ran = false;
    // an earlier call's tables, state and scratch go back first (their sizes follow the options):
    // every call with options starts from the initial state, and none of them grows the net
    {
        void **held[] = {&net->ng_pres_dev, &net->ng_comps_dev, (void **)&net->ng_w32, &net->ng_w16,
                         (void **)&net->ng_sc, (void **)&net->ng_stat, (void **)&net->ng_report,
                         &net->ng_apply_scratch, &net->ng_state_scratch, &net->ng_h};
        for (void **p : held) {
            net->dfree(*p);
            *p = nullptr;
        }
    }
    if (net->ng_comps.empty()) {
        net->ng_on = true;
        return 0;
    }
    const int npre = (int)net->ng_pres.size(), ncomp = (int)net->ng_comps.size();
    const long long ab = kf_ng_apply_scratch_bytes(net->ng_comps.data(), ncomp, net->ng_pres.data(), npre);
    const long long sb = kf_ng_state_scratch_bytes(net->ng_pres.data(), npre);
    if (ab < 0 || sb < 0) {
        set_err(std::string("set_natural_gradient: ") + (kf_last_error() ? kf_last_error() : "scratch size"));
        return -1;
    }
    static_assert(sizeof(KfNgPre) % 4 == 0 && sizeof(KfNgComp) % 4 == 0, "uploaded as 32-bit words");
    net->ng_pres_dev = net->dalloc(npre * sizeof(KfNgPre));
    net->ng_comps_dev = net->dalloc(ncomp * sizeof(KfNgComp));
    net->ng_w32 = (float *)net->dalloc((size_t)w * 4);
    net->ng_w16 = net->dalloc((size_t)h * 2);
    net->ng_sc = (double *)net->dalloc((size_t)s * 8);
    net->ng_stat = (float *)net->dalloc((size_t)st * 4);
    net->ng_report = (float *)net->dalloc((size_t)npre * KF_NG_REPORT * 4);
    net->ng_apply_scratch = net->dalloc((size_t)ab);
    net->ng_state_scratch = net->dalloc((size_t)sb);
    net->ng_h = net->dalloc((size_t)(net->max_T + 1) * max_rp * 2);
    if (!net->ng_pres_dev || !net->ng_comps_dev || !net->ng_w32 || !net->ng_w16 || !net->ng_sc || !net->ng_stat ||
        !net->ng_report || !net->ng_apply_scratch || !net->ng_state_scratch || !net->ng_h ||
        bridge_transfer_int32(net->ng_pres_dev, (const int32_t *)net->ng_pres.data(), npre * sizeof(KfNgPre) / 4) ||
        bridge_transfer_int32(net->ng_comps_dev, (const int32_t *)net->ng_comps.data(), ncomp * sizeof(KfNgComp) / 4)) {
        set_err("set_natural_gradient: alloc / upload of the tables");
        return -1;
    }
    bridge_gpu_memset(net->ng_stat, 0, (size_t)st * 4);
    bridge_gpu_memset(net->ng_report, 0, (size_t)npre * KF_NG_REPORT * 4);
    if (!ck(kf_ng_init(net->ng_pres.data(), (const KfNgPre *)net->ng_pres_dev, npre, &net->ng_opts, net->ng_w32,
                       net->ng_w16, net->ng_sc),
            "set_natural_gradient"))
        return -1;
    net->ng_on = true;
    return 0;
}

extern "C" int nnet_natural_gradient_count(const KfNet *net) {
    return net && net->ng_on ? (int)net->ng_pres.size() : 0;
}

extern "C" int nnet_natural_gradient_stats(KfNet *net, int *component, int *side, float *report, int n) {
    if (!on_device(net, "natural_gradient_stats")) return -1;
    const int npre = nnet_natural_gradient_count(net);
    if (!net->ng_on || !net->ng_ran || n < 0 || n > npre) {
        set_err(!net->ng_on ? "natural_gradient_stats: natural gradient is off"
                : !net->ng_ran ? "natural_gradient_stats: no nnet_backward has run since it was set"
                               : "natural_gradient_stats: more preconditioners asked for than there are");
        return -1;
    }
    // D2H through the bridge, ordered behind the backward on the current stream
    std::vector<float> rep((size_t)npre * KF_NG_REPORT);
    if (npre && bridge_read_fp16((uint16_t *)rep.data(), net->ng_report, rep.size() * 2)) {  // (fp32 = 2x fp16 count)
        set_err("natural_gradient_stats: read");
        return -1;
    }
    for (int i = 0; i < n; ++i) {
        if (component) component[i] = net->ng_pre_comp[i];
        if (side) side[i] = net->ng_pre_side[i];
        if (report) memcpy(report + (size_t)i * KF_NG_REPORT, rep.data() + (size_t)i * KF_NG_REPORT, KF_NG_REPORT * 4);
    }
    return 0;
}

extern "C" int nnet_natural_gradient_state(KfNet *net, int idx, int *component, int *side, int *dim, int *rank,
                                           float *W, double *d, double *rho, double *t) {
    if (!on_device(net, "natural_gradient_state")) return -1;
    if (!net->ng_on || idx < 0 || idx >= (int)net->ng_pres.size()) {
        set_err("natural_gradient_state: natural gradient is off, or no such preconditioner");
        return -1;
    }
    const KfNgPre &p = net->ng_pres[idx];
    if (component) *component = net->ng_pre_comp[idx];
    if (side) *side = net->ng_pre_side[idx];
    if (dim) *dim = p.D;
    if (rank) *rank = p.R;
    std::vector<double> sc(2 + p.R);
    // (fp32 / double reads = 2x / 4x the fp16 count, as nnet_update_stats)
    if ((W && bridge_read_fp16((uint16_t *)W, net->ng_w32 + p.w_off, (size_t)p.R * p.D * 2)) ||
        bridge_read_fp16((uint16_t *)sc.data(), net->ng_sc + p.s_off, sc.size() * 4)) {
        set_err("natural_gradient_state: read");
        return -1;
    }
    if (rho) *rho = sc[0];
    if (t) *t = sc[1];
    if (d) memcpy(d, sc.data() + 2, (size_t)p.R * 8);
    return 0;
}
