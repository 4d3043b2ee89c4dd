// modes.cpp — the switches of the train step and the rules for combining them: the table of
// modes that cannot be combined (admit), implicit dz, row subsampling, the weight-gradient
// stream, the debug hooks, the bound gradient buffer and the data-parallel plan and bind.
#include <cstdlib>

#include "net_internal.h"

// ---------------------------------------------------------------------------
// The modes that cannot all be combined, each pair stated once. A setter (and nnet_backward_n,
// nnet_backward_xent) asks admit() before it switches its mode on; turning a mode off is never refused. A new
// mode is registered here: a value of Mode (net_internal.h), its test in mode_on, its phrase
// and its rows of the table.
// ---------------------------------------------------------------------------
namespace {

// "on" as the passes see it: dropout, SpecAugment, training-mode BatchNorm and self-repair need a
// layer they apply to besides their switch
bool mode_on(const KfNet *net, Mode m) {
    switch (m) {
        case Mode::Fp8: return net->fp8 != 0;
        case Mode::ImplicitDz: return net->implicit_dz != 0;
        case Mode::RowSubsampling: return net->rsub != 0;
        case Mode::NaturalGradient: return net->ng_on;
        case Mode::DataParallel: return net->dp != nullptr;
        case Mode::Dropout: return drop_active(net);
        case Mode::BnTrain: return bnt_active(net);
        case Mode::SpecAugment: return sa_active(net);
        case Mode::LossScale: return net->ls_on;
        case Mode::SelfRepair: return sr_switched(net);
        case Mode::BackwardN:
        case Mode::XentBackward: break;
    }
    return false;
}

// how an error names a mode that is on
const char *phrase(Mode m) {
    switch (m) {
        case Mode::Fp8: return "in MXFP8 mode (nnet_set_fp8)";
        case Mode::ImplicitDz: return "with implicit dz (nnet_set_implicit_dz)";
        case Mode::RowSubsampling: return "with row subsampling (nnet_set_row_subsampling)";
        case Mode::NaturalGradient: return "with natural gradient on (nnet_set_natural_gradient)";
        case Mode::DataParallel: return "on a net bound to data parallel (nnet_bind_dp)";
        case Mode::Dropout: return "with dropout on (nnet_set_dropout)";
        case Mode::BnTrain: return "with training-mode BatchNorm on (nnet_set_bn_train)";
        case Mode::SpecAugment: return "with SpecAugment on (nnet_set_spec_augment)";
        case Mode::LossScale: return "with the loss scale on (nnet_set_loss_scale)";
        case Mode::SelfRepair: return "with ReLU self-repair on (nnet_set_self_repair)";
        case Mode::BackwardN:
        case Mode::XentBackward: break;
    }
    return "";
}

struct Conflict {
    Mode a, b;
    const char *reason;                   // follows the phrase after ": ", or NULL
    std::string (*where)(const KfNet *);  // or: the pair conflicts only where this says why ("": nowhere)
    bool (*lifted)(const KfNet *) = nullptr;  // or: the pair combines while this holds (the text is the plain one otherwise)
};
// nnet_set_bn_train_rows(KF_BN_ROWS_SUBSAMPLED), DESIGN §28: the statistics of a compact layer run
// over the rows c < Tc0, which are rows of the layer
bool bn_rows_subsampled(const KfNet *net) { return net->bnt_rows == KF_BN_ROWS_SUBSAMPLED; }
// (implicit dz x natural gradient is not here: BackwardPass::begin refuses it, no setter does)
const Conflict kConflicts[] = {
    // (self-repair lives in the governed sites' dz, so it is refused where training-mode
    // BatchNorm is. Its switch counts as on from the moment it is set on a net with a layer it can
    // govern, training-mode BatchNorm on or not (sr_switched), and its rows stand first: whichever
    // of the two switches the caller sets second, the text names self-repair.)
    {Mode::SelfRepair, Mode::Fp8, nullptr, nullptr},
    {Mode::SelfRepair, Mode::ImplicitDz, nullptr, nullptr},
    {Mode::SelfRepair, Mode::DataParallel, "the unit statistics would be each rank's own", nullptr},
    {Mode::Fp8, Mode::NaturalGradient, nullptr, nullptr},
    {Mode::Fp8, Mode::Dropout, nullptr, nullptr},
    {Mode::Fp8, Mode::BnTrain, nullptr, nullptr},
    {Mode::Fp8, Mode::SpecAugment, nullptr, sa_mx_conflict},
    {Mode::ImplicitDz, Mode::Dropout, nullptr, nullptr},
    {Mode::ImplicitDz, Mode::BnTrain, nullptr, nullptr},
    // (the compact row set's scratch row and inexact tail rows are not rows of the layer)
    {Mode::RowSubsampling, Mode::BnTrain, nullptr, nullptr, bn_rows_subsampled},
    {Mode::NaturalGradient, Mode::DataParallel, nullptr, nullptr},
    {Mode::DataParallel, Mode::BnTrain, "the statistics would be each rank's own", nullptr},
    // (the Fisher state is not scale-equivariant across a change of the scale; the MXFP8
    // backward has block scales of its own)
    {Mode::LossScale, Mode::NaturalGradient, nullptr, nullptr},
    {Mode::LossScale, Mode::Fp8, nullptr, nullptr},
    {Mode::BackwardN, Mode::SelfRepair, nullptr, nullptr},
    {Mode::BackwardN, Mode::NaturalGradient, nullptr, nullptr},
    {Mode::BackwardN, Mode::Dropout, nullptr, nullptr},
    {Mode::BackwardN, Mode::BnTrain, nullptr, nullptr},
    // (the branch's GEMMs have no MXFP8 form; the bucket plan, backward_groups, walks the chain path)
    {Mode::XentBackward, Mode::Fp8, nullptr, nullptr},
    {Mode::XentBackward, Mode::DataParallel, "the gradient buckets are planned for the chain output's path only", nullptr},
};

}  // namespace

bool admit(KfNet *net, Mode turning_on, const char *fn) {
    for (const Conflict &c : kConflicts) {
        if (c.a != turning_on && c.b != turning_on) continue;
        const Mode other = c.a == turning_on ? c.b : c.a;
        if (!mode_on(net, other) || (c.lifted && c.lifted(net))) continue;
        if (c.where) {
            const std::string why = c.where(net);
            if (why.empty()) continue;
            set_err(std::string(fn) + ": " + phrase(other) + " " + why);
            return false;
        }
        set_err(std::string(fn) + ": not supported " + phrase(other) + (c.reason ? std::string(": ") + c.reason : ""));
        return false;
    }
    return true;
}
extern "C" int nnet_set_implicit_dz(KfNet *net, int on) {
    if (!net) return -1;
    if (on && !admit(net, Mode::ImplicitDz, "set_implicit_dz")) return -1;
    net->implicit_dz = on != 0;
    return 0;
}

extern "C" int nnet_set_row_subsampling(KfNet *net, int stride) {
    if (!on_device(net, "set_row_subsampling")) return -1;
    if (stride == 0 || stride == 1) {
        net->rsub = 0;
        return 0;
    }
    if (stride != 3) {
        set_err("set_row_subsampling: stride " + std::to_string(stride) + " (only 3: chain frame subsampling)");
        return -1;
    }
    if (!admit(net, Mode::RowSubsampling, "set_row_subsampling")) return -1;
    // the top of the output chain whose rows are row-local or 3-strided: TDNN-F with time
    // stride 0 or 3, linear, prefinal, output; consecutive layers. Every layer after the
    // first of them is such a layer too (e.g. Kaldi's xent branch, prefinal-xent and
    // output-xent on prefinal-l), and nothing below reads them.
    const int n = (int)net->layers.size();
    auto row_local = [&](const NetLayer &nl) {
        const Layer &L = nl.L;
        return (L.type == LayerType::TDNNF && (L.time_stride == 0 || L.time_stride == 3)) ||
               (L.type == LayerType::Linear && !nl.per_seq) || L.type == LayerType::Prefinal ||
               L.type == LayerType::Output;
    };
    int first = -1, n3 = 0;
    for (int li = net->chain_out; li >= 0; li = net->layers[li].input) {
        const NetLayer &nl = net->layers[li];
        if (!row_local(nl) || nl.input != li - 1) break;
        first = li;
        if (nl.L.type == LayerType::TDNNF && nl.L.time_stride == 3) ++n3;
    }
    if (first < 0 || net->layers[first].input < 0 || net->layers[net->layers[first].input].L.type != LayerType::ConvReluBN) {
        set_err("set_row_subsampling: needs row-local / 3-strided layers above a conv-relu-batchnorm layer");
        return -1;
    }
    for (int li = first; li < n; ++li)
        if (!row_local(net->layers[li]) || (net->layers[li].input >= 0 && net->layers[li].input < first - 1) ||
            net->layers[li].input2 > -100) {
            set_err("set_row_subsampling: layer " + net->layers[li].L.name + " above the row set is not row-local");
            return -1;
        }
    for (int li = 0; li < first; ++li)
        if (net->layers[li].input >= first || net->layers[li].input2 >= first) {
            set_err("set_row_subsampling: layer " + net->layers[li].L.name + " reads a layer of the row set");
            return -1;
        }
    // tail depth: one row per 3-strided layer and a margin (the scratch row's reach)
    const int nt = n3 + 4;
    const int maxTc = (net->max_T - 1) / 3 + 1 + nt;
    const int din = net->layers[first].L.in_dim;
    if (!net->xc || net->maxTc < maxTc || net->first_c != first) {
        net->xc = net->dalloc((size_t)maxTc * din * 2);
        net->dzc = net->dalloc((size_t)(maxTc + 2) * din * 2);
        net->mc = (uint8_t *)net->dalloc(align_up((size_t)maxTc * din / 8 + 16, 256));
        int maxbn = 0;
        for (int li = first; li < n; ++li)
            if (net->layers[li].L.type == LayerType::TDNNF) maxbn = std::max(maxbn, net->layers[li].L.bottleneck);
        net->rowmask = maxbn ? (uint8_t *)net->dalloc(align_up((size_t)maxTc * maxbn / 8 + 16, 256)) : nullptr;
        net->rm_bn = 0;
        net->rm_tc0 = net->rm_tc = -1;
        if (!net->xc || !net->dzc || !net->mc) {
            set_err("set_row_subsampling: alloc compact buffers");
            return -1;
        }
    }
    for (int li = 0; li < n; ++li) net->layers[li].compact = li >= first;
    net->first_c = first;
    {
        const NetLayer &cl = net->layers[net->layers[first].input];
        const char *ev = getenv("KF_RSUB_CONV");
        // time offsets exactly {-1, 0, 1} and no height subsampling: the input gradient's
        // per-residue GEMMs (backward) cover every input frame
        bool dt3 = !cl.dt.empty();
        for (int e = -1; e <= 1 && dt3; ++e) dt3 = std::find(cl.dt.begin(), cl.dt.end(), e) != cl.dt.end();
        for (int d : cl.dt) dt3 = dt3 && d >= -1 && d <= 1;
        net->conv_c = cl.L.fin > 1 && !cl.kp && cl.L.hsub == 1 && dt3 && !(ev && ev[0] == '0');
        for (int li = 0; li < n; ++li)  // first_c must be the conv output's only reader
            if (li != first && (net->layers[li].input == net->layers[first].input ||
                                net->layers[li].input2 == net->layers[first].input))
                net->conv_c = 0;
        if (net->conv_c) {
            // its weight gradient over the compact rows (BackwardPass::conv_wgrad_compact) reads
            // time-strided rows, which only the 3x3 halo kernel takes, and that kernel does not cover
            // every geometry (e.g. 64 filters at height 20: the strided halo is too large for its
            // four waves): such a conv stays on full rows, read gathered. The plan does not depend
            // on the row count; no launch, so any device pointer serves as the base.
            const Layer &L = cl.L;
            const int rows = ((net->max_T - 1) / 3 + 1) * L.hout;
            KfOperand A = op_im2col(cl, net->dzc, net->max_T, 0);
            A.tmul = 3;
            A.nrows = rows;
            const KfOperand B = op_base(net->dzc, L.fout, rows, L.fout, 0);
            if (kf_gemm_wgrad_halo_applies &&  // (a weak reference, net_internal.h)
                kf_gemm_wgrad_halo_applies((int)cl.dt.size() * L.fin, L.fout, rows, &A, &B) != 1)
                net->conv_c = 0;
        }
    }
    net->rs_nt = nt;
    net->maxTc = maxTc;
    net->rsub = 3;
    return 0;
}

extern "C" int nnet_bn_train_rows(const KfNet *net) { return net ? net->bnt_rows : -1; }

// (no device needed: the policy is a number the switches and the passes read)
extern "C" int nnet_set_bn_train_rows(KfNet *net, int policy) {
    if (!net) return -1;
    if (policy != KF_BN_ROWS_ALL && policy != KF_BN_ROWS_SUBSAMPLED) {
        set_err("set_bn_train_rows: policy=" + std::to_string(policy) + " is not KF_BN_ROWS_ALL or KF_BN_ROWS_SUBSAMPLED");
        return -1;
    }
    if (policy != net->bnt_rows && mode_on(net, Mode::RowSubsampling) && mode_on(net, Mode::BnTrain)) {
        set_err("set_bn_train_rows: not supported with row subsampling (nnet_set_row_subsampling) and training-mode "
                "BatchNorm (nnet_set_bn_train) both on: switch one of them off first");
        return -1;
    }
    net->bnt_rows = policy;
    return 0;
}

extern "C" int nnet_row_set(const KfNet *net, int *tc, int *tc0) {
    if (!net) return -1;
    if (tc) *tc = net->rs.Tc;
    if (tc0) *tc0 = net->rs.Tc0;
    return 0;
}

extern "C" int nnet_debug_backward(KfNet *net, int main_aff, long long stall_cycles) {
    if (!net || main_aff < -1 || main_aff > 2 || stall_cycles < 0) return -1;
    net->main_aff = main_aff;
    net->stall_side = stall_cycles;
    return 0;
}

extern "C" int nnet_debug_alloc_count(const KfNet *net) { return net ? (int)net->allocs.size() : -1; }

extern "C" int nnet_set_wgrad_stream(KfNet *net, int on) {
    if (!net) return -1;
    if (!on && net->wg_stream) bridge_gpu_sync();
    net->wg_side = on != 0 && net->wg_stream != nullptr;
    return 0;
}

// Use caller-owned device memory (>= num_params fp32) as the gradient buffer,
// e.g. a torch tensor handed to the data-parallel all-reduce.
extern "C" int nnet_bind_grad_buffer(KfNet *net, float *dev) {
    if (!on_device(net, "bind_grad_buffer")) return -1;
    if (!dev) {
        set_err("bind_grad_buffer: null");
        return -1;
    }
    net->grad = dev;
    return 0;
}

// ---------------------------------------------------------------------------
// data parallel (kf_dp.h): the backward's parameter groups in the
// order the backward pass (backward.cpp) visits them, cut into all-reduce buckets by kf_dp_plan
// ---------------------------------------------------------------------------
namespace {
// [lo, hi) of the flat buffer written by backward step i (lo = hi: none)
void backward_groups(const KfNet *net, std::vector<long long> &lo, std::vector<long long> &hi) {
    lo.clear();
    hi.clear();
    auto add = [&](const NetLayer &q, long long &a, long long &b) {
        for (int pi : {q.pW, q.pb, q.pW2, q.pb2}) {
            if (pi < 0) continue;
            const ParamRef &p = net->params[pi];
            const long long e = p.off + (long long)align_up((size_t)p.rows * p.cols, 64);
            if (a == b) {
                a = p.off;
                b = e;
            } else {
                a = std::min(a, p.off);
                b = std::max(b, e);
            }
        }
    };
    for (int li = net->chain_out; li >= 0; li = net->layers[li].input) {
        const NetLayer &nl = net->layers[li];
        long long a = 0, b = 0;
        add(nl, a, b);
        if (nl.L.type == LayerType::CombineFeatureMaps)  // the ivector branch is written at this step
            for (int cur = nl.input2; cur >= 0; cur = net->layers[cur].input) add(net->layers[cur], a, b);
        lo.push_back(a);
        hi.push_back(b);
    }
}
}  // namespace

extern "C" int nnet_dp_plan(const KfNet *net, long long bucket_bytes, int max_buckets, int *after_step,
                            long long *begin, long long *end) {
    if (!net || bucket_bytes < 0) {
        set_err("dp_plan: bad arguments");
        return -1;
    }
    std::vector<long long> lo, hi;
    backward_groups(net, lo, hi);
    const int nb = kf_dp_plan((int)lo.size(), lo.data(), hi.data(), net->nparams, bucket_bytes / 4, max_buckets,
                              after_step, begin, end);
    if (nb < 0) set_err(std::string("dp_plan: ") + (kf_dp_last_error() ? kf_dp_last_error() : ""));
    return nb;
}

extern "C" int nnet_bind_dp(KfNet *net, KfDp *dp, long long bucket_bytes) {
    if (!on_device(net, "bind_dp")) return -1;
    net->dp = nullptr;
    net->dp_after.clear();
    net->dp_begin.clear();
    net->dp_end.clear();
    if (!dp) return 0;
    if (!admit(net, Mode::DataParallel, "bind_dp")) return -1;
    std::vector<int> after(256);
    std::vector<long long> b(256), e(256);
    const int nb = nnet_dp_plan(net, bucket_bytes, 256, after.data(), b.data(), e.data());
    if (nb < 0) return -1;
    net->dp_after.assign(after.begin(), after.begin() + nb);
    net->dp_begin.assign(b.begin(), b.begin() + nb);
    net->dp_end.assign(e.begin(), e.begin() + nb);
    net->dp = dp;
    return 0;
}

extern "C" int nnet_dp_debug_early(KfNet *net, int on) {
    if (!net) return -1;
    net->dp_early = on != 0;
    return 0;
}
