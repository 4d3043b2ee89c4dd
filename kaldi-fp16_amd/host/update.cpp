// update.cpp — the parameter steps of the host layer: nnet_sgd, the Kaldi-style update
// (nnet_update) with its tables, and the orthonormal constraint.
#include <cmath>
#include <cstdio>

#include "net_internal.h"

static bool upload_update_tables(KfNet *net);

// The loss scale's part of a parameter step, ahead of the update's first launch: the
// check over the update's segment table and the advance of the state. After it the state says
// whether this step is skipped and holds 1 / the scale the gradient was made with.
static bool loss_scale_check(KfNet *net, const char *what) {
    if (net->upd_dirty && !upload_update_tables(net)) return false;
    return ck(kf_loss_scale_check(net->ls_state, net->grad, net->nparams, (const KfUpdSegment *)net->upd_segs,
                                  net->upd_nseg, (int)net->comps.size(), net->ls_flags),
              what);
}

extern "C" int nnet_sgd(KfNet *net, float lr, float momentum) {
    kf_take_pending(__func__);
    if (!on_device(net, "sgd")) return -1;
    if (net->ls_on && !net->comps.empty()) {
        // (the flat kernel also steps the padding between tensors, as the plain call does)
        if (!loss_scale_check(net, "sgd: loss scale check") ||
            !ck(kf_sgd_flat_scaled(net->master, net->w16, net->grad, net->vel, lr, momentum, net->nparams, net->ls_state),
                "sgd"))
            return -1;
    } else if (!ck(kf_sgd_flat(net->master, net->w16, net->grad, net->vel, lr, momentum, net->nparams), "sgd"))
        return -1;
    net->wt_dirty = true;
    // the MXFP8 weight copies follow every parameter change
    return net->fp8 && !quantise_weights(net, false) ? -1 : 0;
}

// ---------------------------------------------------------------------------
// Kaldi-style update (kf_nnet.h nnet_update): per-component max-change, L2 and
// learning-rate factor over the flat buffers, one kf_update_maxchange call per step
// ---------------------------------------------------------------------------
extern "C" int nnet_num_components(const KfNet *net) { return net ? (int)net->comps.size() : -1; }

extern "C" int nnet_component_info(const KfNet *net, int idx, char *name, int namelen, float *max_change, float *l2,
                                   float *lr_factor, int *first_tensor, int *num_tensors) {
    if (!net || idx < 0 || idx >= (int)net->comps.size()) return -1;
    const UpdComponent &c = net->comps[idx];
    if (name && namelen > 0) snprintf(name, namelen, "%s", c.name.c_str());
    if (max_change) *max_change = c.max_change;
    if (l2) *l2 = c.l2;
    if (lr_factor) *lr_factor = c.lr_factor;
    if (first_tensor) *first_tensor = c.first;
    if (num_tensors) *num_tensors = c.count;
    return 0;
}

extern "C" int nnet_set_component_opts(KfNet *net, const char *name, float max_change, float l2, float lr_factor) {
    if (!net || !name) {
        set_err("set_component_opts: null argument");
        return -1;
    }
    if (!(max_change >= 0) || !(l2 >= 0) || !(lr_factor > 0)) {
        set_err(std::string("set_component_opts: ") + name + " needs max-change >= 0, l2-regularize >= 0 and "
                "learning-rate-factor > 0, got " + std::to_string(max_change) + ", " + std::to_string(l2) + ", " +
                std::to_string(lr_factor));
        return -1;
    }
    for (UpdComponent &c : net->comps)
        if (c.name == name) {
            c.max_change = max_change;
            c.l2 = l2;
            c.lr_factor = lr_factor;
            net->upd_dirty = true;
            return 0;
        }
    set_err(std::string("set_component_opts: no component ") + name);
    return -1;
}

// the device tables of the update: segments once, the components' options whenever they changed
static bool upload_update_tables(KfNet *net) {
    const int ncomp = (int)net->comps.size();
    std::vector<KfUpdSegment> segs;
    std::vector<KfUpdComp> comps(ncomp);
    int wg = 0;
    for (int c = 0; c < ncomp; ++c) {
        const UpdComponent &u = net->comps[c];
        comps[c] = KfUpdComp{u.max_change, u.l2, u.lr_factor, wg, 0};
        for (int pi = u.first; pi < u.first + u.count; ++pi) {
            const ParamRef &p = net->params[pi];
            const long long len = (long long)p.rows * p.cols;
            segs.push_back(KfUpdSegment{p.off, p.off + len, c, wg});
            wg += (int)((len + KF_UPD_CHUNK - 1) / KF_UPD_CHUNK);
        }
        comps[c].num_wg = wg - comps[c].first_wg;
    }
    static_assert(sizeof(KfUpdSegment) % 4 == 0 && sizeof(KfUpdComp) % 4 == 0, "uploaded as 32-bit words");
    if (!net->upd_segs) {
        const long long sb = kf_update_scratch_bytes(net->nparams, (int)segs.size(), ncomp);
        if (sb < 0) {
            set_err("update: scratch size");
            return false;
        }
        net->upd_nseg = (int)segs.size();
        net->upd_segs = net->dalloc(segs.size() * sizeof(KfUpdSegment));
        net->upd_comps = net->dalloc(comps.size() * sizeof(KfUpdComp));
        net->upd_scratch = net->dalloc((size_t)sb);
        net->upd_stats = (float *)net->dalloc((size_t)(2 * ncomp + 2) * 4);
        if (!net->upd_segs || !net->upd_comps || !net->upd_scratch || !net->upd_stats ||
            bridge_transfer_int32(net->upd_segs, (const int32_t *)segs.data(), segs.size() * sizeof(KfUpdSegment) / 4)) {
            net->upd_segs = nullptr;  // (the buffers stay with the net's allocations until it is freed)
            set_err("update: alloc / upload of the segment table");
            return false;
        }
    }
    if (bridge_transfer_int32(net->upd_comps, (const int32_t *)comps.data(), comps.size() * sizeof(KfUpdComp) / 4)) {
        set_err("update: upload of the component table");
        return false;
    }
    net->upd_dirty = false;
    return true;
}

extern "C" int nnet_update(KfNet *net, float lr, float momentum, float max_param_change, float l2_scale) {
    kf_take_pending(__func__);
    if (!on_device(net, "update")) return -1;
    if (!kf_update_maxchange || !kf_update_scratch_bytes) {
        set_err("update: this build of libkaldi_fp16 has no kf_update_maxchange");
        return -1;
    }
    if (!(max_param_change >= 0)) {
        set_err("update: max_param_change must be >= 0");
        return -1;
    }
    if (net->comps.empty()) return 0;
    if (net->upd_dirty && !upload_update_tables(net)) return -1;
    if (net->ls_on) {
        if (!loss_scale_check(net, "update: loss scale check") ||
            !ck(kf_update_maxchange_scaled(net->master, net->w16, net->grad, net->vel, net->nparams,
                                           (const KfUpdSegment *)net->upd_segs, net->upd_nseg,
                                           (const KfUpdComp *)net->upd_comps, (int)net->comps.size(), lr, momentum,
                                           max_param_change, l2_scale, net->upd_scratch, net->upd_stats, net->ls_state),
                "update"))
            return -1;
    } else if (!ck(kf_update_maxchange(net->master, net->w16, net->grad, net->vel, net->nparams,
                                       (const KfUpdSegment *)net->upd_segs, net->upd_nseg,
                                       (const KfUpdComp *)net->upd_comps, (int)net->comps.size(), lr, momentum,
                                       max_param_change, l2_scale, net->upd_scratch, net->upd_stats),
                   "update"))
        return -1;
    net->upd_ran = true;
    net->wt_dirty = true;
    // the MXFP8 weight copies follow every parameter change
    return net->fp8 && !quantise_weights(net, false) ? -1 : 0;
}

extern "C" int nnet_update_stats(KfNet *net, float *norms, float *scales, int n, float *global_norm,
                                 float *global_scale) {
    if (!on_device(net, "update_stats")) return -1;
    const int ncomp = (int)net->comps.size();
    if (!net->upd_ran || n < 0 || n > ncomp) {
        set_err(net->upd_ran ? "update_stats: more components asked for than the network has"
                             : "update_stats: no nnet_update has run");
        return -1;
    }
    // D2H through the bridge, ordered behind the update on the current stream (fp32 read =
    // 2x fp16 count, as nnet_get_params)
    std::vector<float> st((size_t)2 * ncomp + 2);
    if (bridge_read_fp16((uint16_t *)st.data(), net->upd_stats, st.size() * 2)) {
        set_err("update_stats: read");
        return -1;
    }
    for (int c = 0; c < n; ++c) {
        if (norms) norms[c] = st[c];
        if (scales) scales[c] = st[ncomp + c];
    }
    if (global_norm) *global_norm = st[2 * ncomp];
    if (global_scale) *global_scale = st[2 * ncomp + 1];
    return 0;
}

// ---------------------------------------------------------------------------
// Dynamic loss scale (kf_nnet.h nnet_set_loss_scale): the switch and the state; the
// per-step part is loss_scale_check above
// ---------------------------------------------------------------------------
extern "C" int nnet_set_loss_scale(KfNet *net, const KfLossScaleOpts *opts) {
    kf_take_pending(__func__);
    if (!on_device(net, "set_loss_scale")) return -1;
    if (!opts) {
        net->ls_on = false;
        return 0;
    }
    if (!kf_loss_scale_init || !kf_loss_scale_check || !kf_loss_scale_state_bytes || !kf_loss_scale_scratch_bytes ||
        !kf_loss_scale_set_scale || !kf_loss_scale_read || !kf_update_maxchange_scaled || !kf_sgd_flat_scaled ||
        !kf_update_scratch_bytes) {
        set_err("set_loss_scale: this build of libkaldi_fp16 has no loss-scale kernels");
        return -1;
    }
    if (!admit(net, Mode::LossScale, "set_loss_scale")) return -1;
    // everything a step needs is made here: the update's tables, the state and the flags
    if (!net->comps.empty() && net->upd_dirty && !upload_update_tables(net)) return -1;
    if (!net->ls_state) {
        const long long fb = kf_loss_scale_scratch_bytes(net->nparams, net->upd_nseg);
        net->ls_state = net->dalloc((size_t)kf_loss_scale_state_bytes());
        net->ls_flags = fb >= 0 ? net->dalloc((size_t)fb) : nullptr;
        if (!net->ls_state || !net->ls_flags) {
            net->ls_state = nullptr;  // (the buffers stay with the net's allocations until it is freed)
            set_err("set_loss_scale: alloc the state");
            return -1;
        }
    }
    if (!ck(kf_loss_scale_init(net->ls_state, opts), "set_loss_scale")) return -1;
    net->ls_on = true;
    return 0;
}

extern "C" const float *nnet_loss_scale_ptr(const KfNet *net) {
    return net && net->ls_on ? (const float *)net->ls_state : nullptr;
}

extern "C" int nnet_set_loss_scale_value(KfNet *net, float scale) {
    kf_take_pending(__func__);
    if (!on_device(net, "set_loss_scale_value")) return -1;
    if (!net->ls_on) {
        set_err("set_loss_scale_value: the loss scale is off (nnet_set_loss_scale)");
        return -1;
    }
    return ck(kf_loss_scale_set_scale(net->ls_state, scale), "set_loss_scale_value") ? 0 : -1;
}

extern "C" int nnet_loss_scale_stats(KfNet *net, float *scale, int *since, long long *steps, long long *skipped,
                                     int *last_overflow) {
    if (!on_device(net, "loss_scale_stats")) return -1;
    if (!net->ls_on) {
        set_err("loss_scale_stats: the loss scale is off (nnet_set_loss_scale)");
        return -1;
    }
    return ck(kf_loss_scale_read(net->ls_state, scale, since, steps, skipped, last_overflow), "loss_scale_stats") ? 0 : -1;
}

// ---------------------------------------------------------------------------
// Semi-orthogonal constraint (kf_nnet.h nnet_constrain_orthonormal): Kaldi's
// ConstrainOrthonormal over every constrained component, one kf_orthonormal_constrain call
// ---------------------------------------------------------------------------
extern "C" int nnet_component_orthonormal(const KfNet *net, int idx, float *c) {
    if (!net || idx < 0 || idx >= (int)net->comps.size()) return -1;
    if (c) *c = net->comps[idx].orthonormal;
    return 0;
}

// the shapes csrc/orthonormal.hip takes (kf_ops.h): W [K x n], columns constrained
static bool ortho_shape_ok(int K, int n) { return n >= 32 && K % 32 == 0 && n % 32 == 0 && n <= K && n <= 512; }

extern "C" int nnet_set_component_orthonormal(KfNet *net, const char *name, float c) {
    if (!net || !name) {
        set_err("set_component_orthonormal: null argument");
        return -1;
    }
    if (!std::isfinite(c)) {
        set_err(std::string("set_component_orthonormal: ") + name + " needs a finite value");
        return -1;
    }
    for (UpdComponent &u : net->comps) {
        if (u.name != name) continue;
        const ParamRef &p = net->params[u.first];
        if (u.count != 1 || p.rows <= 1) {
            set_err(std::string("set_component_orthonormal: ") + name + " is not a single weight matrix");
            return -1;
        }
        if (c != 0.f && !ortho_shape_ok(p.rows, p.cols)) {
            const std::string shape = std::to_string(p.rows) + " x " + std::to_string(p.cols);
            set_err(std::string("set_component_orthonormal: ") + name + " is " + shape +
                    (p.cols > p.rows ? " (n > K): transposed case not supported"
                                     : ": needs K and n multiples of 32, 32 <= n <= K, n <= 512 (the transposed case "
                                       "not supported either)"));
            return -1;
        }
        u.orthonormal = c;
        net->ort_dirty = true;
        return 0;
    }
    set_err(std::string("set_component_orthonormal: no component ") + name);
    return -1;
}

// the constrained components (c != 0), in nnet_component_info order
static void ortho_list(const KfNet *net, std::vector<int> &idx) {
    idx.clear();
    for (size_t i = 0; i < net->comps.size(); ++i)
        if (net->comps[i].orthonormal != 0.f) idx.push_back((int)i);
}

extern "C" int nnet_orthonormal_components(const KfNet *net, int *idx, int n) {
    if (!net || n < 0) return -1;
    std::vector<int> v;
    ortho_list(net, v);
    return list_get(v, idx, n);
}

// the matrix table, scratch and stats of the constraint: made when the set of constrained
// components or a value changed; device buffers only grow
static bool upload_ortho_table(KfNet *net) {
    ortho_list(net, net->ort_comps);
    net->ort_mats.clear();
    for (int ci : net->ort_comps) {
        const UpdComponent &u = net->comps[ci];
        const ParamRef &p = net->params[u.first];
        if (u.count != 1 || !ortho_shape_ok(p.rows, p.cols)) {
            set_err("constrain_orthonormal: " + u.name + " is " + std::to_string(p.rows) + " x " + std::to_string(p.cols) +
                    ": a constrained matrix needs K and n multiples of 32, 32 <= n <= K, n <= 512 (transposed case "
                    "not supported); set its orthonormal-constraint to 0");
            return false;
        }
        net->ort_mats.push_back(KfOrthoMat{p.off, p.rows, p.cols, u.orthonormal, 0});
    }
    net->ort_ran = false;
    const size_t nm = net->ort_mats.size();
    if (nm == 0) {
        net->ort_dirty = false;
        return true;
    }
    const long long sb = kf_orthonormal_scratch_bytes(net->ort_mats.data(), (int)nm);
    if (sb < 0) {
        set_err("constrain_orthonormal: scratch size");
        return false;
    }
    static_assert(sizeof(KfOrthoMat) % 4 == 0, "uploaded as 32-bit words");
    if (nm > net->ort_cap) {
        net->ort_mats_dev = net->dalloc(nm * sizeof(KfOrthoMat));
        net->ort_stats = (float *)net->dalloc(nm * 4 * sizeof(float));
        net->ort_cap = net->ort_mats_dev && net->ort_stats ? nm : 0;
    }
    if (sb > net->ort_scratch_bytes) {
        net->ort_scratch = net->dalloc((size_t)sb);
        net->ort_scratch_bytes = net->ort_scratch ? sb : 0;
    }
    if (!net->ort_cap || !net->ort_scratch ||
        bridge_transfer_int32(net->ort_mats_dev, (const int32_t *)net->ort_mats.data(), nm * sizeof(KfOrthoMat) / 4)) {
        set_err("constrain_orthonormal: alloc / upload of the matrix table");
        return false;
    }
    net->ort_dirty = false;
    return true;
}

extern "C" int nnet_constrain_orthonormal(KfNet *net) {
    kf_take_pending(__func__);
    if (!on_device(net, "constrain_orthonormal")) return -1;
    if (!kf_orthonormal_constrain || !kf_orthonormal_scratch_bytes) {
        set_err("constrain_orthonormal: this build of libkaldi_fp16 has no kf_orthonormal_constrain");
        return -1;
    }
    if (net->ort_dirty && !upload_ortho_table(net)) return -1;
    if (net->ort_mats.empty()) return 0;  // nothing is constrained: no launch
    if (!ck(kf_orthonormal_constrain(net->master, net->w16, net->nparams, net->ort_mats.data(),
                                     (const KfOrthoMat *)net->ort_mats_dev, (int)net->ort_mats.size(), net->ort_scratch,
                                     net->ort_stats),
            "constrain_orthonormal"))
        return -1;
    net->ort_ran = true;
    net->wt_dirty = true;
    // the MXFP8 weight copies follow every parameter change
    return net->fp8 && !quantise_weights(net, false) ? -1 : 0;
}

extern "C" int nnet_orthonormal_stats(KfNet *net, float *scale, float *ratio, float *err, int n) {
    if (!on_device(net, "orthonormal_stats")) return -1;
    const int nm = (int)net->ort_mats.size();
    if (!net->ort_ran || n < 0 || n > nm) {
        set_err(net->ort_ran ? "orthonormal_stats: more components asked for than are constrained"
                             : "orthonormal_stats: no nnet_constrain_orthonormal has run");
        return -1;
    }
    // D2H through the bridge, ordered behind the call on the current stream (fp32 read = 2x
    // fp16 count, as nnet_update_stats)
    std::vector<float> st((size_t)4 * nm);
    if (bridge_read_fp16((uint16_t *)st.data(), net->ort_stats, st.size() * 2)) {
        set_err("orthonormal_stats: read");
        return -1;
    }
    for (int i = 0; i < n; ++i) {
        if (scale) scale[i] = st[4 * i];
        if (ratio) ratio[i] = st[4 * i + 1];
        if (err) err[i] = st[4 * i + 2];
    }
    return 0;
}
