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
// Training-mode BatchNorm of the TDNN-F layers (kf_nnet.h nnet_set_bn_train): the
// switch, the statistics and the commit. forward.cpp normalises by the batch statistics,
// backward.cpp differentiates through them.
// ---------------------------------------------------------------------------
static NetLayer *bnt_layer(KfNet *net, const char *layer, int which, const char *what) {
    NetLayer *nl = which == 0 ? find_layer(net, layer) : nullptr;
    if (nl && std::count(net->bnt_layers.begin(), net->bnt_layers.end(), (int)(nl - net->layers.data()))) return nl;
    set_err(std::string(what) + ": training-mode BatchNorm (nnet_set_bn_train) does not govern BatchNorm '" +
            std::to_string(which) + "' of layer " + (layer ? layer : "(null)"));
    return nullptr;
}

extern "C" int nnet_bn_train_layers(const KfNet *net, int *idx, int n) {
    return net ? list_get(net->bnt_layers, idx, n) : -1;
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
    int maxw = 0;
    for (int li : net->bnt_layers) maxw = std::max(maxw, net->layers[li].L.out_dim);
    if (!net->bnt_ab) {  // the first time: r, the batch statistics and the accumulators of every layer
        for (int li : net->bnt_layers) {
            NetLayer &nl = net->layers[li];
            const size_t D = (size_t)nl.L.out_dim;
            if (D % 8 || !nl.mask) {
                set_err("set_bn_train: layer " + nl.L.name + " needs out_dim % 8 == 0 and a ReLU mask");
                return -1;
            }
            nl.bnt_r = net->dalloc((size_t)net->max_T * D * 2);
            nl.bnt_stat = (float *)net->dalloc(4 * D * 4);
            nl.bnt_acc = (double *)net->dalloc((2 + 2 * D) * 8);
            if (!nl.bnt_r || !nl.bnt_stat || !nl.bnt_acc) {
                set_err("set_bn_train: alloc " + nl.L.name);
                return -1;
            }
            bridge_gpu_memset(nl.bnt_stat, 0, 4 * D * 4);
            bridge_gpu_memset(nl.bnt_acc, 0, (2 + 2 * D) * 8);
        }
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
    NetLayer *nl = bnt_layer(net, layer, which, "bn_batch_stats");
    if (!nl) return -1;
    if (!nl->bnt_act || !nl->bnt_stat) {
        set_err(std::string("bn_batch_stats: the last forward did not run ") + layer + " in training mode");
        return -1;
    }
    const size_t D = (size_t)nl->L.out_dim;
    // (ordered behind the forward on the current stream, and synchronises; fp32 read = 2x fp16 count)
    if ((mean && bridge_read_fp16((uint16_t *)mean, nl->bnt_stat, 2 * D)) ||
        (var && bridge_read_fp16((uint16_t *)var, nl->bnt_stat + D, 2 * D))) {
        set_err("bn_batch_stats: read");
        return -1;
    }
    return 0;
}

// (ordered behind the forward on the current stream, and synchronises; a double read = 4x fp16 count)
static bool bnt_read_acc(NetLayer &nl, std::vector<double> &h) {
    h.assign(2 + 2 * (size_t)nl.L.out_dim, 0.0);
    return !nl.bnt_acc || bridge_read_fp16((uint16_t *)h.data(), nl.bnt_acc, h.size() * 4) == 0;
}

extern "C" int nnet_bn_stats(KfNet *net, const char *layer, int which, double *count, double *sum, double *sumsq) {
    if (!on_device(net, "bn_stats")) return -1;
    NetLayer *nl = bnt_layer(net, layer, which, "bn_stats");
    if (!nl) return -1;
    std::vector<double> h;
    if (!bnt_read_acc(*nl, h)) {
        set_err("bn_stats: read");
        return -1;
    }
    const size_t D = (size_t)nl->L.out_dim;
    if (count) *count = h[0];
    if (sum) std::copy(h.begin() + 2, h.begin() + 2 + D, sum);
    if (sumsq) std::copy(h.begin() + 2 + D, h.end(), sumsq);
    return 0;
}

extern "C" int nnet_bn_zero_stats(KfNet *net) {
    if (!on_device(net, "bn_zero_stats")) return -1;
    for (int li : net->bnt_layers) {
        NetLayer &nl = net->layers[li];
        if (nl.bnt_acc) bridge_gpu_memset(nl.bnt_acc, 0, (2 + 2 * (size_t)nl.L.out_dim) * 8);
    }
    return 0;
}

extern "C" int nnet_bn_commit(KfNet *net) {
    if (!on_device(net, "bn_commit")) return -1;
    int n = 0;
    std::vector<double> h;
    for (int li : net->bnt_layers) {
        NetLayer &nl = net->layers[li];
        if (!nl.bnt_acc) continue;
        if (!bnt_read_acc(nl, h)) {
            set_err("bn_commit: read");
            return -1;
        }
        if (!(h[0] > 0.0)) continue;
        const size_t D = (size_t)nl.L.out_dim;
        std::vector<float> mean(D), var(D), gamma(D, 1.f), beta(D, 0.f);
        for (size_t c = 0; c < D; ++c) {
            const double mu = h[2 + c] / h[0], v = h[2 + D + c] / h[0] - mu * mu;
            mean[c] = (float)mu;
            var[c] = (float)(v > 0.0 ? v : 0.0);
        }
        if (nnet_set_bn(net, nl.L.name.c_str(), 0, mean.data(), var.data(), gamma.data(), beta.data(), nl.bn_eps,
                        nl.bn_rms) != 0)
            return -1;
        ++n;
    }
    return n;
}
