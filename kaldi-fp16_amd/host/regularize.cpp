// regularize.cpp — the train-time regularisers of the host layer: the sequences they draw
// per, per-sequence dropout, SpecAugment and training-mode BatchNorm (switches, getters, commit).
#include "net_internal.h"

// ---------------------------------------------------------------------------
// Per-sequence dropout of the TDNN-F layers (kf_nnet.h nnet_set_dropout): the
// switches and tables. forward.cpp draws the masks and hands them to the affine GEMM's
// epilogue, backward.cpp to the input-gradient GEMM that produces the layer's dz.
// ---------------------------------------------------------------------------
extern "C" int nnet_set_sequences(KfNet *net, const int *seq_row0, int B) {
    if (!net) {
        set_err("set_sequences: null network");
        return -1;
    }
    if (!seq_row0 && B == 0) {  // back to one sequence
        net->seq_row0.clear();
        return 0;
    }
    if (!seq_row0 || B <= 0 || seq_row0[0] != 0 || seq_row0[B] <= 0 || seq_row0[B] > net->max_T || B > seq_row0[B]) {
        set_err("set_sequences: needs B in [1, T], seq_row0[0] = 0 and T = seq_row0[B] in (0, max_frames]");
        return -1;
    }
    for (int s = 0; s < B; ++s)
        if (seq_row0[s + 1] <= seq_row0[s]) {
            set_err("set_sequences: empty or unordered sequence " + std::to_string(s));
            return -1;
        }
    if (net->master) {  // (a layout-only net keeps the host copy only)
        if (!net->seq_off && !(net->seq_off = (int *)net->dalloc(((size_t)net->max_T + 1) * 4))) {
            set_err("set_sequences: alloc seq offsets");
            return -1;
        }
        if (bridge_transfer_int32(net->seq_off, seq_row0, (size_t)B + 1)) {
            set_err("set_sequences: upload seq offsets");
            return -1;
        }
    }
    net->seq_row0.assign(seq_row0, seq_row0 + B + 1);
    return 0;
}

extern "C" int nnet_dropout_layers(const KfNet *net, int *idx, int n) {
    return net ? list_get(net->drop_layers, idx, n) : -1;
}

extern "C" int nnet_set_dropout_proportion(KfNet *net, const char *layer, float p) {
    if (!net) {
        set_err("set_dropout_proportion: null network");
        return -1;
    }
    if (!(p >= 0.f && p <= 0.5f)) {
        set_err("set_dropout_proportion: the proportion must be in [0, 0.5], got " + std::to_string(p));
        return -1;
    }
    if (!layer) {
        for (int li : net->drop_layers) net->layers[li].drop_p = p;
        return 0;
    }
    NetLayer *nl = find_layer(net, layer);
    if (!nl || nl->drop_ord < 0) {
        set_err(std::string("set_dropout_proportion: ") + (nl ? "layer " : "no layer ") + layer +
                (nl ? " has no dropout component" : ""));
        return -1;
    }
    nl->drop_p = p;
    return 0;
}

extern "C" int nnet_dropout_proportion(const KfNet *net, const char *layer, float *p) {
    if (const NetLayer *nl = find_layer(const_cast<KfNet *>(net), layer)) {
        if (p) *p = nl->drop_ord < 0 ? -1.f : nl->drop_p;
        return 0;
    }
    set_err(std::string("dropout_proportion: no layer ") + (layer ? layer : "(null)"));
    return -1;
}

extern "C" int nnet_set_dropout(KfNet *net, int on, unsigned long long seed) {
    if (!net) {
        set_err("set_dropout: null network");
        return -1;
    }
    if (on && !net->drop_layers.empty()) {
        if (!admit(net, Mode::Dropout, "set_dropout")) return -1;
        if (net->drop_layers.size() > 65535) {
            set_err("set_dropout: too many dropout layers");
            return -1;
        }
    }
    net->drop_on = on != 0;
    net->drop_seed = seed;
    return 0;
}

extern "C" int nnet_set_dropout_step(KfNet *net, long long step) {
    if (!net || step < 0 || step > 0xFFFFFFFFll) {
        set_err("set_dropout_step: the step must be in [0, 2^32)");
        return -1;
    }
    net->drop_step = step;
    return 0;
}

extern "C" long long nnet_dropout_step(const KfNet *net) { return net ? net->drop_step : -1; }

extern "C" int nnet_dropout_mask(KfNet *net, const char *layer, float *host, int *B, int *dim) {
    if (!on_device(net, "dropout_mask")) return -1;
    const NetLayer *nl = find_layer(net, layer);
    if (!nl) {
        set_err(std::string("dropout_mask: no layer ") + (layer ? layer : "(null)"));
        return -1;
    }
    if (nl->drop_ord < 0 || !nl->drop_act || !nl->drop) {
        set_err(std::string("dropout_mask: the last forward drew no mask for ") + layer +
                (nl->drop_ord < 0 ? " (no dropout component)" : " (dropout off or proportion 0)"));
        return -1;
    }
    if (B) *B = net->drop_B;
    if (dim) *dim = nl->L.out_dim;
    // (ordered behind the forward on the current stream, and synchronises; fp32 read = 2x
    // fp16 count, as nnet_update_stats)
    if (host && bridge_read_fp16((uint16_t *)host, nl->drop, (size_t)net->drop_B * nl->L.out_dim * 2)) {
        set_err("dropout_mask: read");
        return -1;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// SpecAugment of the spec-augment layers (kf_nnet.h nnet_set_spec_augment): the
// switch, the options and the step. forward.cpp draws and applies the masks.
// ---------------------------------------------------------------------------
static NetLayer *sa_layer(KfNet *net, const char *layer, const char *what) {
    NetLayer *nl = find_layer(net, layer);
    if (nl && nl->sa_ord >= 0) return nl;
    set_err(nl ? std::string(what) + ": layer " + layer + " is not a spec-augment-layer"
               : std::string(what) + ": no layer " + (layer ? layer : "(null)"));
    return nullptr;
}

extern "C" int nnet_spec_augment_layers(const KfNet *net, int *idx, int n) {
    return net ? list_get(net->sa_layers, idx, n) : -1;
}

extern "C" int nnet_spec_augment_opts(const KfNet *net, const char *layer, double *f, double *z, int *m) {
    const NetLayer *nl = sa_layer(const_cast<KfNet *>(net), layer, "spec_augment_opts");
    if (!nl) return -1;
    if (f) *f = nl->sa_f;
    if (z) *z = nl->sa_z;
    if (m) *m = nl->sa_m;
    return 0;
}

extern "C" int nnet_set_spec_augment_opts(KfNet *net, const char *layer, double f, double z, int m) {
    NetLayer *nl = sa_layer(net, layer, "set_spec_augment_opts");
    if (!nl) return -1;
    if (!(f >= 0.0 && f <= 1.0) || !(z >= 0.0 && z < 1.0) || m < 1) {
        set_err("set_spec_augment_opts: needs freq-max-proportion in [0, 1], time-zeroed-proportion in [0, 1) and "
                "time-mask-max-frames >= 1, got " + std::to_string(f) + ", " + std::to_string(z) + ", " + std::to_string(m));
        return -1;
    }
    nl->sa_f = f;
    nl->sa_z = z;
    nl->sa_m = m;
    return 0;
}

extern "C" int nnet_set_spec_augment(KfNet *net, int on, unsigned long long seed) {
    if (!net) {
        set_err("set_spec_augment: null network");
        return -1;
    }
    if (on && !net->sa_layers.empty() && !admit(net, Mode::SpecAugment, "set_spec_augment")) return -1;
    net->sa_on = on != 0;
    net->sa_seed = seed;
    return 0;
}

extern "C" int nnet_set_spec_augment_step(KfNet *net, long long step) {
    if (!net || step < 0 || step > 0xFFFFFFFFll) {
        set_err("set_spec_augment_step: the step must be in [0, 2^32)");
        return -1;
    }
    net->sa_step = step;
    return 0;
}

extern "C" long long nnet_spec_augment_step(const KfNet *net) { return net ? net->sa_step : -1; }

extern "C" int nnet_spec_augment_rows(KfNet *net, const char *layer, int32_t *host, int *T) {
    if (!on_device(net, "spec_augment_rows")) return -1;
    NetLayer *nl = sa_layer(net, layer, "spec_augment_rows");
    if (!nl) return -1;
    if (!nl->sa_act || !nl->sa_rows) {
        set_err(std::string("spec_augment_rows: the last forward drew no mask for ") + layer +
                " (SpecAugment off, or no band and no time mask)");
        return -1;
    }
    if (T) *T = net->T;
    // (ordered behind the forward on the current stream, and synchronises; int32 read = 2x fp16
    // count, as nnet_dropout_mask)
    if (host && bridge_read_fp16((uint16_t *)host, nl->sa_rows, (size_t)net->T * 2)) {
        set_err("spec_augment_rows: read");
        return -1;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Training-mode BatchNorm (kf_nnet.h nnet_set_bn_train): the sites, the
// switch, the statistics and the commit. forward.cpp normalises by the batch statistics,
// backward.cpp differentiates through them.
// ---------------------------------------------------------------------------
static int bnt_site_of(LayerType t) {
    switch (t) {
        case LayerType::TDNNF: return KF_BN_SITE_TDNNF;
        case LayerType::ConvReluBN: return KF_BN_SITE_CONV;
        case LayerType::Prefinal: return KF_BN_SITE_PREFINAL;
        case LayerType::Batchnorm: return KF_BN_SITE_COMPONENT;
        default: return 0;  // (the attention layer's BatchNorm is fused into its kernel: never governed)
    }
}

// a governed BatchNorm's storage: r, the statistics and the accumulators (NULL: `which` is not one
// of the layer's BatchNorms)
struct BntSlot {
    void **r;
    float **stat;
    double **acc;
    int dim;
    float eps, rms;
};
static bool bnt_slot(NetLayer &nl, int which, BntSlot &s) {
    const bool pre = nl.L.type == LayerType::Prefinal;
    if (which < 0 || which > (pre && nl.has_bn2 ? 1 : 0)) return false;
    if (which) s = BntSlot{&nl.bnt_r2, &nl.bnt_stat2, &nl.bnt_acc2, bnt_dim(nl, 1), nl.bn2_eps, nl.bn2_rms};
    else s = BntSlot{&nl.bnt_r, &nl.bnt_stat, &nl.bnt_acc, bnt_dim(nl, 0), nl.bn_eps, nl.bn_rms};
    return true;
}

static NetLayer *bnt_layer(KfNet *net, const char *layer, int which, const char *what, BntSlot &slot) {
    NetLayer *nl = find_layer(net, layer);
    if (nl && std::count(net->bnt_layers.begin(), net->bnt_layers.end(), (int)(nl - net->layers.data())) &&
        bnt_slot(*nl, which, slot))
        return nl;
    set_err(std::string(what) + ": training-mode BatchNorm (nnet_set_bn_train) does not govern BatchNorm '" +
            std::to_string(which) + "' of layer " + (layer ? layer : "(null)"));
    return nullptr;
}

extern "C" int nnet_bn_train_layers(const KfNet *net, int *idx, int n) {
    return net ? list_get(net->bnt_layers, idx, n) : -1;
}

extern "C" int nnet_bn_train_sites(const KfNet *net) { return net ? net->bnt_sites : -1; }

extern "C" int nnet_set_bn_train_sites(KfNet *net, int sites) {
    if (!net) return -1;
    if (sites < 0 || (sites & ~KF_BN_SITE_ALL)) {
        set_err("set_bn_train_sites: sites=" + std::to_string(sites) + " is not a mask of KF_BN_SITE_*");
        return -1;
    }
    if (bnt_active(net)) {
        set_err("set_bn_train_sites: not supported with training-mode BatchNorm on (nnet_set_bn_train): switch it off first");
        return -1;
    }
    auto apply = [net](int m) {
        net->bnt_sites = m;
        net->bnt_layers.clear();
        for (size_t i = 0; i < net->layers.size(); ++i) {
            net->layers[i].bnt_act = false;
            if (bnt_site_of(net->layers[i].L.type) & m) net->bnt_layers.push_back((int)i);
        }
    };
    const int old = net->bnt_sites;
    apply(sites);
    // the switch was set while it governed nothing (no such layer under the old sites): it now
    // goes on for the new ones, with everything nnet_set_bn_train checks and allocates
    if (net->bnt_on && !net->bnt_layers.empty()) {
        net->bnt_on = 0;
        if (nnet_set_bn_train(net, 1) != 0) {
            apply(old);
            net->bnt_on = 1;
            return -1;
        }
    }
    return 0;
}

extern "C" int nnet_bn_dim(const KfNet *net, const char *layer, int which) {
    NetLayer *nl = find_layer(const_cast<KfNet *>(net), layer);
    BntSlot slot;
    if (nl && bnt_site_of(nl->L.type) && bnt_slot(*nl, which, slot)) return slot.dim;
    if (nl && nl->L.type == LayerType::Attention && which == 0) return nl->L.out_dim;
    set_err(std::string("bn_dim: no BatchNorm '") + std::to_string(which) + "' in layer " + (layer ? layer : "(null)"));
    return -1;
}

// a frame-level batchnorm-component above a trainable layer: its backward is a scale folded into
// the producing epilogue (backward.cpp dx_epilogue), which the batch statistics cannot be
static const NetLayer *bnt_unsupported_component(const KfNet *net) {
    for (int li : net->bnt_layers) {
        const NetLayer &nl = net->layers[li];
        if (nl.L.type == LayerType::Batchnorm && !nl.per_seq && nl.needs_dx) return &nl;
    }
    return nullptr;
}

extern "C" int nnet_set_bn_train(KfNet *net, int on) {
    if (!on_device(net, "set_bn_train")) return -1;
    if (!on || net->bnt_layers.empty()) {
        net->bnt_on = on != 0;
        return 0;
    }
    if (!admit(net, Mode::BnTrain, "set_bn_train")) return -1;
    if (!kf_bn_train_stats) {
        set_err("set_bn_train: this build of libkaldi_fp16 has no training-mode BatchNorm kernels");
        return -1;
    }
    if ((net->bnt_sites & KF_BN_SITE_CONV) && (!kf_bn_block_stats || !kf_bn_block_bwd_stats)) {
        set_err("set_bn_train: this build of libkaldi_fp16 has no block BatchNorm kernels");
        return -1;
    }
    if (const NetLayer *bad = bnt_unsupported_component(net)) {
        set_err("set_bn_train: batchnorm-component " + bad->L.name +
                " lies above a trainable layer on the frame level; training mode is not supported there "
                "(nnet_set_bn_train_sites without KF_BN_SITE_COMPONENT)");
        return -1;
    }
    int maxw = 0;
    for (int li : net->bnt_layers)
        for (int which = 0; which < 2; ++which) {
            BntSlot s;
            if (bnt_slot(net->layers[li], which, s)) maxw = std::max(maxw, s.dim);
        }
    // the first time a layer is governed: r, the batch statistics and the accumulators
    for (int li : net->bnt_layers) {
        NetLayer &nl = net->layers[li];
        for (int which = 0; which < 2; ++which) {
            BntSlot s;
            if (!bnt_slot(nl, which, s) || *s.stat) continue;
            const size_t D = (size_t)s.dim;
            const bool relu = nl.L.type != LayerType::Batchnorm && which == 0;
            if (D % 8 || (relu && !nl.mask)) {
                set_err("set_bn_train: layer " + nl.L.name + " needs out_dim % 8 == 0 and a ReLU mask");
                return -1;
            }
            // r as wide as the tensor the BatchNorm sees (a conv layer: every height of it); a
            // batchnorm-component reads its input in place: a per-sequence one keeps the backward's
            // dz here (its rows are at most max_T), a frame-level one has no backward and no r
            const size_t w = nl.L.type == LayerType::ConvReluBN ? (size_t)nl.L.out_dim : D;
            const bool need_r = nl.L.type != LayerType::Batchnorm || nl.per_seq;
            if (need_r) *s.r = net->dalloc((size_t)net->max_T * w * 2);
            *s.stat = (float *)net->dalloc(4 * D * 4);
            *s.acc = (double *)net->dalloc((2 + 2 * D) * 8);
            if ((need_r && !*s.r) || !*s.stat || !*s.acc) {
                set_err("set_bn_train: alloc " + nl.L.name);
                return -1;
            }
            bridge_gpu_memset(*s.stat, 0, 4 * D * 4);
            bridge_gpu_memset(*s.acc, 0, (2 + 2 * D) * 8);
        }
    }
    if (maxw > net->bnt_w) {  // (grows when the sites changed between two switches: the old pair goes back)
        net->dfree(net->bnt_ab);
        net->bnt_w = 0;
        if (!(net->bnt_ab = (float *)net->dalloc((size_t)2 * maxw * 4))) {
            set_err("set_bn_train: alloc backward columns");
            return -1;
        }
        net->bnt_w = maxw;
    }
    net->bnt_on = 1;
    return 0;
}

extern "C" int nnet_bn_batch_stats(KfNet *net, const char *layer, int which, float *mean, float *var) {
    if (!on_device(net, "bn_batch_stats")) return -1;
    BntSlot s;
    NetLayer *nl = bnt_layer(net, layer, which, "bn_batch_stats", s);
    if (!nl) return -1;
    if (!nl->bnt_act || !*s.stat) {
        set_err(std::string("bn_batch_stats: the last forward did not run ") + layer + " in training mode");
        return -1;
    }
    const size_t D = (size_t)s.dim;
    // (ordered behind the forward on the current stream, and synchronises; fp32 read = 2x fp16 count)
    if ((mean && bridge_read_fp16((uint16_t *)mean, *s.stat, 2 * D)) ||
        (var && bridge_read_fp16((uint16_t *)var, *s.stat + D, 2 * D))) {
        set_err("bn_batch_stats: read");
        return -1;
    }
    return 0;
}

// (ordered behind the forward on the current stream, and synchronises; a double read = 4x fp16 count)
static bool bnt_read_acc(const BntSlot &s, std::vector<double> &h) {
    h.assign(2 + 2 * (size_t)s.dim, 0.0);
    return !*s.acc || bridge_read_fp16((uint16_t *)h.data(), *s.acc, h.size() * 4) == 0;
}

extern "C" int nnet_bn_stats(KfNet *net, const char *layer, int which, double *count, double *sum, double *sumsq) {
    if (!on_device(net, "bn_stats")) return -1;
    BntSlot s;
    NetLayer *nl = bnt_layer(net, layer, which, "bn_stats", s);
    if (!nl) return -1;
    std::vector<double> h;
    if (!bnt_read_acc(s, h)) {
        set_err("bn_stats: read");
        return -1;
    }
    const size_t D = (size_t)s.dim;
    if (count) *count = h[0];
    if (sum) std::copy(h.begin() + 2, h.begin() + 2 + D, sum);
    if (sumsq) std::copy(h.begin() + 2 + D, h.end(), sumsq);
    return 0;
}

extern "C" int nnet_bn_zero_stats(KfNet *net) {
    if (!on_device(net, "bn_zero_stats")) return -1;
    for (int li : net->bnt_layers)
        for (int which = 0; which < 2; ++which) {
            BntSlot s;
            if (bnt_slot(net->layers[li], which, s) && *s.acc) bridge_gpu_memset(*s.acc, 0, (2 + 2 * (size_t)s.dim) * 8);
        }
    return 0;
}

// returns the layers committed (a prefinal layer counts once, both of its BatchNorms committed)
extern "C" int nnet_bn_commit(KfNet *net) {
    if (!on_device(net, "bn_commit")) return -1;
    int n = 0;
    std::vector<double> h;
    for (int li : net->bnt_layers) {
        NetLayer &nl = net->layers[li];
        bool any = false;
        for (int which = 0; which < 2; ++which) {
            BntSlot s;
            if (!bnt_slot(nl, which, s) || !*s.acc) continue;
            if (!bnt_read_acc(s, h)) {
                set_err("bn_commit: read");
                return -1;
            }
            if (!(h[0] > 0.0)) continue;
            const size_t D = (size_t)s.dim;
            std::vector<float> mean(D), var(D), gamma(D, 1.f), beta(D, 0.f);
            for (size_t c = 0; c < D; ++c) {
                const double mu = h[2 + c] / h[0], v = h[2 + D + c] / h[0] - mu * mu;
                mean[c] = (float)mu;
                var[c] = (float)(v > 0.0 ? v : 0.0);
            }
            if (nnet_set_bn(net, nl.L.name.c_str(), which, mean.data(), var.data(), gamma.data(), beta.data(), s.eps, s.rms) != 0)
                return -1;
            any = true;
        }
        n += any;
    }
    return n;
}

// ---------------------------------------------------------------------------
// ReLU unit statistics and self-repair (kf_nnet.h nnet_set_self_repair): the switch,
// the sites' storage and table, the options and the read-backs. forward.cpp counts through the
// _relu statistics entries, backward.cpp builds the repair vectors and adds them to the sites' dz.
// ---------------------------------------------------------------------------
// the table of net->sr_sites (kf_ops.h KfRepairSite) from the layers' options, on the host and on
// the device; a blocking copy, so ordered behind every launch that read the old one
static bool sr_upload(KfNet *net, const char *fn) {
    const size_t n = net->sr_sites.size();
    net->sr_tab.clear();
    for (int li : net->sr_sites) {
        const NetLayer &nl = net->layers[li];
        net->sr_tab.push_back(KfRepairSite{nl.sr_acc, nl.sr_acc + 2, nl.sr_s, bnt_dim(nl, 0), nl.sr_scale, nl.sr_lower, nl.sr_upper});
    }
    net->sr_dirty = true;  // (until the device holds it)
    if (n > net->sr_tab_cap) {
        net->dfree(net->sr_tab_dev);
        net->sr_tab_cap = 0;
        if (!(net->sr_tab_dev = net->dalloc(n * sizeof(KfRepairSite)))) {
            set_err(std::string(fn) + ": alloc self-repair table");
            return false;
        }
        net->sr_tab_cap = n;
    }
    if (n && bridge_transfer_int32(net->sr_tab_dev, (const int32_t *)net->sr_tab.data(), n * sizeof(KfRepairSite) / 4)) {
        set_err(std::string(fn) + ": upload self-repair table");
        return false;
    }
    net->sr_dirty = false;
    return true;
}

bool sr_prepare(KfNet *net, const char *fn) {
    for (NetLayer &nl : net->layers) nl.sr_act = false;
    if (!sr_active(net)) return true;
    if (!admit(net, Mode::SelfRepair, fn)) return false;
    if (!kf_bn_train_stats_relu || !kf_bn_block_stats_relu || !kf_relu_repair_vectors || !kf_bn_train_bwd_apply_repair ||
        !kf_bn_train_bwd_apply_rows_repair) {
        set_err(std::string(fn) + ": this build of libkaldi_fp16 has no self-repair kernels");
        return false;
    }
    // the sites of this forward against the table's, without a list of their own: nothing is
    // allocated on a step that finds the table as it left it
    auto is_site = [net](int li) { return sr_site_type(net->layers[li].L.type) && net->layers[li].bnt_stat != nullptr; };
    size_t ns = 0;
    bool same = !net->sr_dirty;
    for (int li : net->bnt_layers) {
        if (!is_site(li)) continue;
        same = same && ns < net->sr_sites.size() && net->sr_sites[ns] == li;
        ++ns;
    }
    if (!same || ns != net->sr_sites.size()) {
        net->sr_sites.clear();
        for (int li : net->bnt_layers)
            if (is_site(li)) net->sr_sites.push_back(li);
        // the first time a layer is a site: its accumulators and repair vector
        for (int li : net->sr_sites) {
            NetLayer &nl = net->layers[li];
            if (nl.sr_acc) continue;
            const size_t D = (size_t)bnt_dim(nl, 0);
            nl.sr_acc = (double *)net->dalloc((2 + D) * 8);
            nl.sr_s = (float *)net->dalloc(D * 4);
            if (!nl.sr_acc || !nl.sr_s) {
                nl.sr_acc = nullptr;  // (the buffers stay with the net's allocations until it is freed)
                net->sr_sites.clear();
                set_err(std::string(fn) + ": alloc self-repair " + nl.L.name);
                return false;
            }
            bridge_gpu_memset(nl.sr_acc, 0, (2 + D) * 8);
            bridge_gpu_memset(nl.sr_s, 0, D * 4);
        }
        if (!sr_upload(net, fn)) return false;
    }
    for (int li : net->sr_sites) net->layers[li].sr_act = true;
    return true;
}

extern "C" int nnet_set_self_repair(KfNet *net, int on) {
    if (!on_device(net, "set_self_repair")) return -1;
    if (!on) {
        net->sr_on = 0;
        return 0;
    }
    const int old = net->sr_on;
    net->sr_on = 1;
    // (where no site exists the switch is accepted and changes nothing, like dropout's)
    if ((sr_switched(net) && !admit(net, Mode::SelfRepair, "set_self_repair")) || !sr_prepare(net, "set_self_repair")) {
        net->sr_on = old;
        return -1;
    }
    for (NetLayer &nl : net->layers) nl.sr_act = false;  // (the next forward's to set)
    return 0;
}

extern "C" int nnet_self_repair_sites(const KfNet *net, int *idx, int n) {
    if (!net) return -1;
    std::vector<int> sites;
    if (sr_active(net))  // (sr_prepare's rule)
        for (int li : net->bnt_layers)
            if (sr_site_type(net->layers[li].L.type) && net->layers[li].bnt_stat) sites.push_back(li);
    return list_get(sites, idx, n);
}

static NetLayer *sr_layer(KfNet *net, const char *layer, const char *what) {
    NetLayer *nl = find_layer(net, layer);
    if (nl && sr_site_type(nl->L.type)) return nl;
    set_err(std::string(what) + ": layer " + (layer ? layer : "(null)") + " has no ReLU that self-repair applies to");
    return nullptr;
}

extern "C" int nnet_self_repair_opts(const KfNet *net, const char *layer, float *scale, double *lower, double *upper) {
    NetLayer *nl = sr_layer(const_cast<KfNet *>(net), layer, "self_repair_opts");
    if (!nl) return -1;
    if (scale) *scale = nl->sr_scale;
    if (lower) *lower = nl->sr_lower;
    if (upper) *upper = nl->sr_upper;
    return 0;
}

extern "C" int nnet_set_self_repair_opts(KfNet *net, const char *layer, float scale, double lower, double upper) {
    NetLayer *nl = sr_layer(net, layer, "set_self_repair_opts");
    if (!nl) return -1;
    if (!(scale >= 0.f) || !(lower >= 0.0 && lower < upper && upper <= 1.0)) {
        set_err("set_self_repair_opts: needs scale >= 0 and 0 <= lower < upper <= 1");
        return -1;
    }
    nl->sr_scale = scale;
    nl->sr_lower = lower;
    nl->sr_upper = upper;
    // a table that holds the layer follows at once: a backward after this call uses the new options
    const int li = (int)(nl - net->layers.data());
    if (std::count(net->sr_sites.begin(), net->sr_sites.end(), li) && !sr_upload(net, "set_self_repair_opts")) return -1;
    return 0;
}

// the site's storage, or NULL with the error set: the mode never counted in this layer
static NetLayer *sr_counted(KfNet *net, const char *layer, const char *what) {
    NetLayer *nl = sr_layer(net, layer, what);
    if (nl && nl->sr_acc) return nl;
    if (nl) set_err(std::string(what) + ": self-repair (nnet_set_self_repair) never governed layer " + layer);
    return nullptr;
}

// (ordered behind the forward on the current stream, and synchronises; a double read = 4x fp16 count)
extern "C" int nnet_relu_stats(KfNet *net, const char *layer, double *count, double *value_sum, double *deriv_sum) {
    if (!on_device(net, "relu_stats")) return -1;
    NetLayer *nl = sr_counted(net, layer, "relu_stats");
    if (!nl) return -1;
    const size_t D = (size_t)bnt_dim(*nl, 0);
    std::vector<double> h(2 + D);
    if (bridge_read_fp16((uint16_t *)h.data(), nl->sr_acc, h.size() * 4) ||
        (value_sum && bridge_read_fp16((uint16_t *)value_sum, nl->bnt_acc + 2, D * 4))) {
        set_err("relu_stats: read");
        return -1;
    }
    if (count) *count = h[0];
    if (deriv_sum) std::copy(h.begin() + 2, h.end(), deriv_sum);
    return 0;
}

extern "C" int nnet_relu_zero_stats(KfNet *net) {
    if (!on_device(net, "relu_zero_stats")) return -1;
    for (NetLayer &nl : net->layers)
        if (nl.sr_acc) bridge_gpu_memset(nl.sr_acc, 0, (2 + (size_t)bnt_dim(nl, 0)) * 8);
    return nnet_bn_zero_stats(net);
}

extern "C" int nnet_self_repair_vector(KfNet *net, const char *layer, float *host) {
    if (!on_device(net, "self_repair_vector")) return -1;
    NetLayer *nl = sr_counted(net, layer, "self_repair_vector");
    if (!nl || !host) return -1;
    if (bridge_read_fp16((uint16_t *)host, nl->sr_s, 2 * (size_t)bnt_dim(*nl, 0))) {
        set_err("self_repair_vector: read");
        return -1;
    }
    return 0;
}
