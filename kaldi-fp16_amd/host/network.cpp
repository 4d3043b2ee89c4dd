// network.cpp — the network of the C++ host layer: topology, allocation, parameters and their
// setters (mxfp8.cpp, modes.cpp, update.cpp, natgrad.cpp, regularize.cpp: the switches and the
// parameter steps; forward.cpp / backward.cpp: the passes).
//
// Together they restate internal/nnet/forward.go (Network.Forward and the per-layer
// forward functions), internal/nnet/network_backward.go (Network.Backward) and
// internal/gpu/optimize.go (SGDOptimizer) on top of the MI355X C-ABI:
//   * every dense product is one kf_gemm_fused / kf_gemm_wgrad launch whose
//     operand addressing does the TDNN splice (forward.go:699-790) and the conv
//     im2col (forward.go:435-456) implicitly, with bias / ReLU / BatchNorm /
//     bypass fused into the epilogue;
//   * backward is the exact gradient of that forward (the reference's
//     backwardTDNNF / backwardPrefinal are not);
//   * all trainable parameters live in one flat fp32 master / fp16 working /
//     fp32 gradient / fp32 velocity allocation, so the optimiser is one launch
//     and the data-parallel gradient exchange is one contiguous buffer.
// Memory comes from the bridge_* ABI, as the Go layer does (internal/gpu/tensor.go).
#include <cstdlib>
#include <cmath>
#include <functional>
#include <cstdio>
#include <memory>

#include "net_internal.h"

static __thread char g_nnet_err[1024];
void set_err(const std::string &s) { snprintf(g_nnet_err, sizeof g_nnet_err, "%s", s.c_str()); }
extern "C" const char *nnet_last_error(void) { return g_nnet_err[0] ? g_nnet_err : nullptr; }

bool ck(int rc, const char *what) {
    if (rc != 0) {
        const char *e = kf_last_error();
        if (!e) e = kf_layers_last_error();
        if (!e) e = ops_last_error();
        set_err(std::string(what) + ": " + (e ? e : "failed"));
        return false;
    }
    return true;
}

// a network from nnet_create_layout has no device storage
bool on_device(const KfNet *net, const char *what) {
    if (net && net->master) return true;
    set_err(std::string(what) + ": " + (net ? "layout-only network (nnet_create_layout)" : "null network"));
    return false;
}

NetLayer *find_layer(KfNet *net, const char *name) {
    if (net && name)
        for (auto &nl : net->layers)
            if (nl.L.name == name) return &nl;
    return nullptr;
}

namespace {

// makeIDCTMatrix, forward.go:1190-1210
std::vector<float> idct_matrix(int dim, double lifter) {
    std::vector<float> m((size_t)dim * dim);
    for (int i = 0; i < dim; ++i)
        for (int j = 0; j < dim; ++j) {
            double v = cos(M_PI * j * (i + 0.5) / dim);
            v *= j == 0 ? sqrt(1.0 / dim) : sqrt(2.0 / dim);
            if (lifter > 0 && j > 0) v *= 1.0 + (lifter / 2.0) * sin(M_PI * j / lifter);
            m[(size_t)i * dim + j] = (float)v;
        }
    return m;
}

// truncating fp32 -> fp16, internal/gpu/tensor.go:158-173 (weights enter this way)
uint16_t f32_to_f16_trunc(float f) {
    uint32_t bits;
    memcpy(&bits, &f, 4);
    uint16_t sign = (uint16_t)((bits >> 16) & 0x8000u);
    int exp = (int)((bits >> 23) & 0xFF) - 127;
    uint32_t frac = bits & 0x7FFFFFu;
    if (exp > 15) return sign | 0x7C00u;
    if (exp < -14) return sign;
    return (uint16_t)(sign | (uint16_t)((exp + 15) << 10) | (uint16_t)(frac >> 13));
}
float f16_to_f32(uint16_t h) {
    uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1Fu, frac = h & 0x3FFu;
    uint32_t bits;
    if (exp == 0) {
        if (frac == 0) bits = sign;
        else {
            exp = 1;
            while (!(frac & 0x400u)) {
                frac <<= 1;
                exp--;
            }
            frac &= 0x3FFu;
            bits = sign | ((uint32_t)(127 - 15 + (int)exp) << 23) | (frac << 13);
        }
    } else if (exp == 31) {
        bits = sign | 0x7F800000u | (frac << 13);
    } else {
        bits = sign | ((exp - 15 + 127) << 23) | (frac << 13);
    }
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

int add_param(KfNet *net, const std::string &name, int rows, int cols) {
    ParamRef p{name, rows, cols, net->nparams};
    net->params.push_back(p);
    net->nparams += (long long)align_up((size_t)rows * cols, 64);
    return (int)net->params.size() - 1;
}

// fold frozen BN into per-column scale/shift, expanded to `width` columns by
// repeating the `dim` pattern (conv layers: width = hout*fout, dim = fout)
bool upload_bn(KfNet *net, const std::vector<float> *h, float eps, float rms, int dim, int width,
               float *&dscale, float *&dshift) {
    std::vector<float> sc(width), sh(width);
    for (int c = 0; c < width; ++c) {
        int d = c % dim;
        float inv = 1.0f / sqrtf(h[1][d] + eps);
        float s = rms != 1.0f ? rms * inv : h[2][d] * inv;
        sc[c] = s;
        sh[c] = (rms != 1.0f ? 0.f : h[3][d]) - h[0][d] * s;
    }
    if (!dscale) {
        dscale = (float *)net->dalloc(width * 4);
        dshift = (float *)net->dalloc(width * 4);
        if (!dscale || !dshift) return false;
    }
    return bridge_transfer_float32(dscale, sc.data(), width) == 0 &&
           bridge_transfer_float32(dshift, sh.data(), width) == 0;
}

void identity_bn(std::vector<float> *h, int dim) {  // identityBN, forward.go:1172-1187
    h[0].assign(dim, 0.f);
    h[1].assign(dim, 1.f);
    h[2].assign(dim, 1.f);
    h[3].assign(dim, 0.f);
}

}  // namespace

// Parse, resolve and lay out the network on the host: layers, inputs, the flat
// parameter layout, the backward path. No device work (nnet_create_layout).
// device = false (nnet_create_layout): the MI355X kernels' shape constraints (dims that
// are multiples of 8 / 32, IDCT <= 64) are not enforced; the layout does not depend on them.
static bool build_topology(KfNet *net, const char *xconfig_text, int max_frames, bool device) {
    std::vector<kf::LayerConfig> cfgs;
    std::string err;
    if (!kf::ParseXConfig(xconfig_text ? xconfig_text : "", cfgs, err) ||
        !kf::ResolveLayers(cfgs, net->all, err)) {
        set_err("parse xconfig: " + err);
        return false;
    }
    if (max_frames <= 0) {
        set_err("max_frames must be positive");
        return false;
    }
    net->max_T = max_frames;
    std::map<std::string, int> index;  // layer name -> index in net->layers (-1 = input)
    for (const Layer &L : net->all) {
        if (L.type == LayerType::Input) {
            if (L.name == "ivector") {  // per-sequence input (Kaldi's ivector-dim input)
                if (net->ivec_dim) {
                    set_err("more than one ivector input");
                    return false;
                }
                net->ivec_dim = L.out_dim;
                index[L.name] = -2;
                continue;
            }
            if (net->feat_dim) {
                set_err("more than one frame-level input layer (only 'input' and 'ivector' are supported)");
                return false;
            }
            net->feat_dim = L.out_dim;
            index[L.name] = -1;
            continue;
        }
        NetLayer nl;
        nl.L = L;
        nl.sr_scale = (float)L.self_repair_scale;  // (nnet_set_self_repair; read on tdnnf, prefinal and conv layers)
        nl.sr_lower = L.self_repair_lower;
        nl.sr_upper = L.self_repair_upper;
        auto is_seq = [&](int idx) { return idx == -2 || (idx >= 0 && net->layers[idx].per_seq); };
        auto dim_of = [&](int idx) {
            return idx == -2 ? net->ivec_dim : idx >= 0 ? net->layers[idx].L.out_dim : net->feat_dim;
        };
        if (L.input.kind == kf::InputRef::Append && L.type != LayerType::CombineFeatureMaps) {
            // General Append(a, b, ...) (forward.go:264-310: column concat of the inputs, in
            // order; network_backward.go:147-170 splits the gradient back). Each further
            // part is appended by a hidden combine-feature-maps node of height 1, which
            // is exactly a column concat [a | b] with b broadcast to the frames of its
            // sequence when b is per-sequence (an ivector given per frame is B = T
            // sequences of one frame: the reference's [T x dim] ivector Append).
            if (L.input_names.size() < 2) {
                set_err("layer " + L.name + ": Append needs two or more inputs");
                return false;
            }
            std::vector<int> parts;
            for (const auto &nm : L.input_names) {
                auto it = index.find(nm);
                if (it == index.end()) {
                    set_err("layer " + L.name + ": Append input " + nm + " not found");
                    return false;
                }
                parts.push_back(it->second);
            }
            if (is_seq(parts[0])) {
                set_err("layer " + L.name + ": the first Append input must be frame-level");
                return false;
            }
            int cur = parts[0];
            for (size_t k = 1; k < parts.size(); ++k) {
                NetLayer hc;
                hc.L.type = LayerType::CombineFeatureMaps;
                hc.L.name = L.name + ".append" + (parts.size() > 2 ? std::to_string(k) : std::string());
                hc.L.height = 1;
                hc.L.nf1 = dim_of(cur);
                hc.L.nf2 = dim_of(parts[k]);
                hc.L.in_dim = hc.L.out_dim = hc.L.nf1 + hc.L.nf2;
                hc.L.input.kind = kf::InputRef::Append;
                hc.input = cur;
                hc.input2 = parts[k];
                net->layers.push_back(hc);
                index[hc.L.name] = cur = (int)net->layers.size() - 1;
            }
            nl.L.input.kind = kf::InputRef::Simple;
            nl.L.input_names = {net->layers[cur].L.name};
        }
        if (nl.L.input.kind == kf::InputRef::Append) {
            // only combine-feature-maps takes an Append, of a frame-level and a per-sequence
            // (or frame-level) input (Kaldi's Append(idct-batchnorm, ivector-batchnorm))
            if (L.type != LayerType::CombineFeatureMaps || L.input_names.size() != 2) {
                set_err("layer " + L.name + ": Append is supported as the input of combine-feature-maps, of two layers");
                return false;
            }
            auto a = index.find(L.input_names[0]), b = index.find(L.input_names[1]);
            if (a == index.end() || b == index.end() || is_seq(a->second)) {
                set_err("layer " + L.name + ": Append inputs not found, or the first one is per-sequence");
                return false;
            }
            nl.input = a->second;
            nl.input2 = b->second;
        } else {
            if (nl.L.input_names.size() != 1) {
                set_err("layer " + L.name + ": one input expected");
                return false;
            }
            auto it = index.find(nl.L.input_names[0]);
            if (it == index.end()) {
                set_err("layer " + L.name + ": input not found");
                return false;
            }
            nl.input = it->second;
            // ReplaceIndex(x, t, 0) of a per-sequence source, or anything fed by one
            nl.per_seq = is_seq(nl.input);
            if (nl.per_seq && L.type != LayerType::Linear && L.type != LayerType::Batchnorm) {
                set_err("layer " + L.name + ": only linear-component and batchnorm-component run on the "
                        "per-sequence (ivector) branch");
                return false;
            }
        }
        if (L.type == LayerType::CombineFeatureMaps) {
            const int da = nl.input < 0 ? net->feat_dim : net->layers[nl.input].L.out_dim;
            const int db = nl.input2 == -2 ? net->ivec_dim
                           : nl.input2 >= 0 ? net->layers[nl.input2].L.out_dim : net->feat_dim;
            if (nl.input2 == -100 || L.height <= 0 || da != L.height * L.nf1 || db != L.height * L.nf2) {
                set_err("combine-feature-maps " + L.name + ": needs Append(a, b) with dims height*num-filters1 "
                        "and height*num-filters2");
                return false;
            }
        }
        const int din = L.in_dim, dout = L.out_dim;
        const std::string &n = L.name;
        switch (L.type) {
            case LayerType::IDCT:
                if (din != dout || (device && (din > 64 || din % 8))) {
                    set_err("idct-layer " + n + ": dim must equal input dim, <= 64, multiple of 8");
                    return false;
                }
                break;
            case LayerType::Batchnorm:
                identity_bn(nl.hbn, dout);
                nl.bn_rms = (float)L.target_rms;
                break;
            case LayerType::ConvReluBN: {
                if (L.hin <= 0 || L.fin <= 0 || L.fin * L.hin != din || (device && L.fout % 8)) {
                    set_err("conv layer " + n + ": inconsistent height-in / filters");
                    return false;
                }
                for (int a : L.time_offsets)
                    for (int b : L.height_offsets) {
                        nl.dt.push_back(a);
                        nl.dh.push_back(b);
                    }
                if (nl.dt.empty() || nl.dt.size() > KF_MAX_PARTS) {
                    set_err("conv layer " + n + ": need 1..9 (time x height) offsets");
                    return false;
                }
                if (L.fin != 1 && L.fin % 32) {  // small fin: im2col + GEMM (csrc/ivector.hip)
                    nl.kp = (int)((nl.dt.size() * L.fin + 63) / 64 * 64);
                }
                const int K = (int)nl.dt.size() * L.fin;
                nl.pW = add_param(net, n + ".W", K, L.fout);
                nl.pb = add_param(net, n + ".Bias", 1, L.fout);
                identity_bn(nl.hbn, L.fout);
                break;
            }
            case LayerType::TDNNF: {
                const int s = L.time_stride, bn = L.bottleneck;
                if (device && (bn % 32 || din % 32 || dout % 8)) {
                    set_err("tdnnf layer " + n + ": dims must be multiples of 32");
                    return false;
                }
                nl.pW = add_param(net, n + ".LinearW", s > 0 ? 2 * din : din, bn);
                nl.pW2 = add_param(net, n + ".AffineW", s > 0 ? 2 * bn : bn, dout);
                nl.pb2 = add_param(net, n + ".AffineBias", 1, dout);
                nl.bypass = L.bypass_scale > 0 && din == dout;
                identity_bn(nl.hbn, dout);
                net->bnt_layers.push_back((int)net->layers.size());  // (nnet_set_bn_train governs it)
                if (L.dropout_proportion >= 0) {  // the layer has a dropout component
                    nl.drop_p = (float)L.dropout_proportion;
                    nl.drop_ord = (int)net->drop_layers.size();
                    net->drop_layers.push_back((int)net->layers.size());
                }
                break;
            }
            case LayerType::Linear:
                nl.pW = add_param(net, n + ".W", din, dout);
                break;
            case LayerType::Prefinal:
                nl.pW = add_param(net, n + ".BigW", din, L.big_dim);
                nl.pb = add_param(net, n + ".BigBias", 1, L.big_dim);
                nl.pW2 = add_param(net, n + ".SmallW", L.big_dim, L.small_dim);
                identity_bn(nl.hbn, L.big_dim);
                identity_bn(nl.hbn2, L.small_dim);
                nl.has_bn2 = true;
                break;
            case LayerType::Output:
                if (L.include_log_softmax) {
                    // the xent branch (log-softmax output) is a "next" row
                }
                nl.pW = add_param(net, n + ".W", din, dout);
                nl.pb = add_param(net, n + ".Bias", 1, dout);
                break;
            case LayerType::Attention: {
                const int ctx = 1 + L.num_left + L.num_right, A = att_affine(L);
                if (L.num_heads <= 0 || L.key_dim <= 0 || L.value_dim < 0 || L.att_stride <= 0 ||
                    (device && (ctx > 64 || L.num_heads * ctx > 1024 || A % 8 || dout % 8 || din % 8))) {
                    set_err("attention layer " + n + ": needs heads > 0, key-dim > 0, context <= 64, "
                            "heads*context <= 1024 and affine / output / input dims multiples of 8");
                    return false;
                }
                nl.pW = add_param(net, n + ".W", din, A);
                nl.pb = add_param(net, n + ".Bias", 1, A);
                nl.key_scale = L.key_scale > 0 ? (float)L.key_scale : (float)(1.0 / sqrt((double)L.key_dim));
                identity_bn(nl.hbn, dout);
                break;
            }
            case LayerType::SpecAugment:
                if (device && dout > 32767) {  // (kf_specaug_rows packs the band into 2 x 15 bits)
                    set_err("spec-augment layer " + n + ": dim above 32767");
                    return false;
                }
                nl.sa_f = L.freq_max_proportion;
                nl.sa_z = L.time_zeroed_proportion;
                nl.sa_m = L.time_mask_max_frames;
                nl.sa_ord = (int)net->sa_layers.size();
                net->sa_layers.push_back((int)net->layers.size());
                break;
            case LayerType::CombineFeatureMaps:
                break;
            default:
                set_err("layer " + n + ": type not supported on the MI355X path");
                return false;
        }
        // the layer's update components (kf_nnet.h nnet_update): one per Kaldi nnet3 component,
        // under the name nnet_load_kaldi reads it by, with the layer's options
        auto comp = [&](const std::string &cname, int first, int count) {
            net->comps.push_back(UpdComponent{cname, first, count, (float)L.max_change, (float)L.l2_regularize,
                                              (float)L.lr_factor, 0.f});
        };
        // the one weight matrix the layer's orthonormal-constraint applies to
        auto comp_orth = [&](const std::string &cname, int first) {
            comp(cname, first, 1);
            net->comps.back().orthonormal = (float)L.orthonormal;
        };
        switch (L.type) {
            case LayerType::ConvReluBN:
                comp(n + ".conv", nl.pW, 2);
                break;
            case LayerType::TDNNF:
                comp_orth(n + ".linear", nl.pW);
                comp(n + ".affine", nl.pW2, 2);
                break;
            case LayerType::Linear:
                comp_orth(n, nl.pW);
                break;
            case LayerType::Prefinal: {
                const std::string pre = n.find("xent") != std::string::npos ? "prefinal-xent" : "prefinal-chain";
                comp(pre + ".affine", nl.pW, 2);
                comp_orth(pre + ".linear", nl.pW2);
                break;
            }
            case LayerType::Output:
            case LayerType::Attention:
                comp(n + ".affine", nl.pW, 2);
                break;
            default:
                break;
        }
        index[L.name] = (int)net->layers.size();
        net->layers.push_back(nl);
    }
    if (net->layers.empty()) {
        set_err("no layers");
        return false;
    }
    for (size_t i = 0; i < net->layers.size() && net->chain_out < 0; ++i)
        if (net->layers[i].L.type == LayerType::Output && net->layers[i].L.name == "output") net->chain_out = (int)i;
    for (size_t i = 0; i < net->layers.size() && net->chain_out < 0; ++i)
        if (net->layers[i].L.type == LayerType::Output) net->chain_out = (int)i;
    if (net->chain_out < 0) net->chain_out = (int)net->layers.size() - 1;
    {
        std::vector<char> on(net->layers.size(), 0);
        for (int cur = net->chain_out; cur >= 0; cur = net->layers[cur].input) on[cur] = 1;
        for (size_t i = 0; i < net->layers.size(); ++i) {
            if (on[i]) continue;
            const NetLayer &nl = net->layers[i];
            for (int pi : {nl.pW, nl.pb, nl.pW2, nl.pb2})
                if (pi >= 0) net->offpath.emplace_back(net->params[pi].off, (long long)net->params[pi].rows * net->params[pi].cols);
        }
    }
    // which layers need an input gradient (a trainable layer lies below them)
    {
        // a trainable layer lies below idx, along inputs and combine-feature-maps' second input
        std::function<bool(int)> below = [&](int idx) -> bool {
            if (idx < 0) return false;
            const NetLayer &q = net->layers[idx];
            return is_trainable(q.L.type) || below(q.input) || (q.input2 >= 0 && below(q.input2));
        };
        for (size_t i = 0; i < net->layers.size(); ++i) net->layers[i].needs_dx = below(net->layers[i].input);
    }
    return true;
}

// Device storage of a laid-out network: parameters, activations, masks, BN, scratch.
static bool alloc_device(KfNet *net, int max_frames) {
    // flat parameter storage
    const long long P = net->nparams > 0 ? net->nparams : 64;
    net->master = (float *)net->dalloc(P * 4);
    net->grad = (float *)net->dalloc(P * 4);
    net->vel = (float *)net->dalloc(P * 4);
    net->w16 = net->dalloc(P * 2);
    if (!net->master || !net->grad || !net->vel || !net->w16) {
        set_err("alloc params: " + std::string(bridge_last_error() ? bridge_last_error() : ""));
        return false;
    }
    bridge_gpu_memset(net->master, 0, P * 4);
    bridge_gpu_memset(net->grad, 0, P * 4);
    bridge_gpu_memset(net->vel, 0, P * 4);
    bridge_gpu_memset(net->w16, 0, P * 2);
    // activations, masks, BN params
    const size_t T = (size_t)max_frames;
    size_t maxw = 16;
    for (auto &nl : net->layers) {
        const Layer &L = nl.L;
        const int dout = L.out_dim;
        maxw = std::max(maxw, (size_t)std::max(L.in_dim, dout));
        if (L.type == LayerType::SpecAugment) {
            nl.act_alias = true;
        } else {
            nl.act = net->dalloc(T * dout * 2);
            if (!nl.act) {
                set_err("alloc activation " + L.name);
                return false;
            }
        }
        int mwidth = 0;
        if (L.type == LayerType::ConvReluBN || L.type == LayerType::TDNNF || L.type == LayerType::Attention)
            mwidth = dout;
        if (L.type == LayerType::Attention) {
            const int A = att_affine(L), ctx = 1 + L.num_left + L.num_right;
            nl.aux = net->dalloc((size_t)T * A * 2);
            nl.dproj = net->dalloc((size_t)T * A * 2);
            nl.att_scratch = (float *)net->dalloc((size_t)2 * T * L.num_heads * ctx * 4);
            if (!nl.aux || !nl.dproj || !nl.att_scratch) {
                set_err("alloc attention buffers");
                return false;
            }
        }
        if (L.type == LayerType::ConvReluBN && nl.kp) {
            nl.im2col = net->dalloc((size_t)T * L.hout * nl.kp * 2);
            nl.wpad = net->dalloc((size_t)nl.kp * L.fout * 2);
            nl.gwpad = (float *)net->dalloc((size_t)nl.kp * L.fout * 4);
            if (!nl.im2col || !nl.wpad || !nl.gwpad) {
                set_err("alloc small-fin conv buffers");
                return false;
            }
            bridge_gpu_memset(nl.wpad, 0, (size_t)nl.kp * L.fout * 2);
        }
        if (L.type == LayerType::CombineFeatureMaps && nl.input2 != -100) {
            nl.gdb = net->dalloc((size_t)T * L.height * L.nf2 * 2);
            if (!nl.gdb) {
                set_err("alloc combine gradient");
                return false;
            }
        }
        if (L.type == LayerType::Prefinal) mwidth = L.big_dim;
        if (mwidth) nl.mask = (uint8_t *)net->dalloc(align_up(T * mwidth / 8 + 16, 256));
        if (L.type == LayerType::TDNNF) nl.aux = net->dalloc(T * L.bottleneck * 2);
        if (L.type == LayerType::Prefinal) {
            nl.aux = net->dalloc(T * L.big_dim * 2);
            maxw = std::max(maxw, (size_t)L.big_dim);
        }
        if (L.type == LayerType::IDCT) {
            auto m = idct_matrix(dout, L.cepstral_lifter);
            std::vector<uint16_t> h(m.size());
            for (size_t i = 0; i < m.size(); ++i) h[i] = f32_to_f16_trunc(m[i]);
            nl.idct = net->dalloc(h.size() * 2);
            if (bridge_transfer_fp16(nl.idct, h.data(), h.size())) {
                set_err("upload idct");
                return false;
            }
        }
        if (L.type == LayerType::Batchnorm &&
            !upload_bn(net, nl.hbn, nl.bn_eps, nl.bn_rms, dout, dout, nl.bn_scale, nl.bn_shift))
            return false;
        if (L.type == LayerType::ConvReluBN &&
            !upload_bn(net, nl.hbn, nl.bn_eps, 1.f, L.fout, dout, nl.bn_scale, nl.bn_shift))
            return false;
        if ((L.type == LayerType::TDNNF || L.type == LayerType::Attention) &&
            !upload_bn(net, nl.hbn, nl.bn_eps, 1.f, dout, dout, nl.bn_scale, nl.bn_shift))
            return false;
        if (L.type == LayerType::Prefinal &&
            (!upload_bn(net, nl.hbn, nl.bn_eps, 1.f, L.big_dim, L.big_dim, nl.bn_scale,
                        nl.bn_shift) ||
             !upload_bn(net, nl.hbn2, nl.bn2_eps, 1.f, L.small_dim, L.small_dim,
                        nl.bn2_scale, nl.bn2_shift)))
            return false;
    }
    // transposed copies of the short-K forward weights (TDNN-F affine, prefinal big)
    for (auto &nl : net->layers) {
        const Layer &L = nl.L;
        int pi = -1, K = 0, N = 0;
        if (L.type == LayerType::TDNNF) {
            pi = nl.pW2;
            K = L.time_stride > 0 ? 2 * L.bottleneck : L.bottleneck;
            N = L.out_dim;
        } else if (L.type == LayerType::Prefinal) {
            pi = nl.pW;
            K = L.in_dim;
            N = L.big_dim;
        }
        if (pi < 0 || K > 512 || K % 32 || N % 32) continue;
        nl.wt = net->dalloc((size_t)K * N * 2);
        if (!nl.wt) {
            set_err("alloc transposed weights " + L.name);
            return false;
        }
        nl.wt_pi = pi;
        nl.wt_K = K;
        nl.wt_N = N;
    }
    // gradient buffers carry two spare rows for the splice-transpose edge sums
    for (int i = 0; i < 3; ++i) {
        net->dz[i] = net->dalloc((T + 2) * maxw * 2);
        net->g[i] = net->dalloc((T + 2) * maxw * 2);
    }
    net->dbott = net->dalloc((T + 2) * maxw * 2);
    net->dbott2 = net->dalloc((T + 2) * maxw * 2);
    net->dbott3 = net->dalloc((T + 2) * maxw * 2);
    {
        size_t w2 = 0;
        for (auto &nl : net->layers)
            if (nl.L.type == LayerType::TDNNF)
                w2 = std::max(w2, (size_t)(nl.L.time_stride > 0 ? 2 : 1) * nl.L.bottleneck * nl.L.out_dim * 2);
        net->w2s = w2 ? net->dalloc(w2) : nullptr;
        if (w2 && !net->w2s) {
            set_err("alloc backward scratch");
            return false;
        }
    }
    net->edge_half = align_up(maxw * 2, 256);
    net->edge = net->dalloc(net->edge_half * 2);
    if (!net->dz[0] || !net->dz[1] || !net->dz[2] || !net->g[0] || !net->g[1] || !net->g[2] || !net->dbott ||
        !net->dbott2 || !net->dbott3 || !net->edge) {
        set_err("alloc backward scratch");
        return false;
    }
    net->wg_stream = kf_stream_new();
    net->hp_stream = kf_stream_new_high();
    net->ev_go = kf_event_new();
    net->ev_side = kf_event_new();
    for (auto &e : net->ev_step) e = kf_event_new();
    net->ev_aux = kf_event_new();
    if (!net->wg_stream || !net->ev_go || !net->ev_side || !net->ev_step[0] || !net->ev_step[1] || !net->ev_step[2] ||
        !net->ev_aux) {
        set_err("create the weight-gradient stream");
        return false;
    }
    return true;
}

extern "C" KfNet *nnet_create(const char *xconfig_text, int max_frames) {
    g_nnet_err[0] = 0;
    std::unique_ptr<KfNet> net(new KfNet);
    if (!build_topology(net.get(), xconfig_text, max_frames, true) || !alloc_device(net.get(), max_frames))
        return nullptr;
    return net.release();
}

extern "C" KfNet *nnet_create_layout(const char *xconfig_text, int max_frames) {
    g_nnet_err[0] = 0;
    std::unique_ptr<KfNet> net(new KfNet);
    if (!build_topology(net.get(), xconfig_text, max_frames, false)) return nullptr;
    return net.release();
}

extern "C" void nnet_free(KfNet *net) {
    kf_take_pending(__func__);
    delete net;
    kf_take_pending("the return of nnet_free");  // a stream / event / free call that failed
}

extern "C" int nnet_num_layers(const KfNet *net) { return (int)net->layers.size(); }

extern "C" int nnet_layer_info(const KfNet *net, int idx, char *name, int namelen, int *type,
                               int *in_dim, int *out_dim) {
    if (idx < 0 || idx >= (int)net->layers.size()) return -1;
    const Layer &L = net->layers[idx].L;
    if (name && namelen > 0) snprintf(name, namelen, "%s", L.name.c_str());
    if (type) *type = (int)L.type;
    if (in_dim) *in_dim = L.in_dim;
    if (out_dim) *out_dim = L.out_dim;
    return 0;
}

extern "C" long long nnet_num_params(const KfNet *net) { return net->nparams; }
extern "C" int nnet_num_param_tensors(const KfNet *net) { return (int)net->params.size(); }
extern "C" int nnet_param_info(const KfNet *net, int idx, char *name, int namelen, int *rows,
                               int *cols, long long *offset) {
    if (idx < 0 || idx >= (int)net->params.size()) return -1;
    const ParamRef &p = net->params[idx];
    if (name && namelen > 0) snprintf(name, namelen, "%s", p.name.c_str());
    if (rows) *rows = p.rows;
    if (cols) *cols = p.cols;
    if (offset) *offset = p.off;
    return 0;
}

extern "C" int nnet_set_params(KfNet *net, const float *host) {
    if (!on_device(net, "set_params")) return -1;
    const long long P = net->nparams;
    std::vector<uint16_t> h(P, 0);
    std::vector<float> m(P, 0.f);
    for (const ParamRef &p : net->params)
        for (long long i = 0; i < (long long)p.rows * p.cols; ++i) {
            uint16_t v = f32_to_f16_trunc(host[p.off + i]);
            h[p.off + i] = v;
            m[p.off + i] = f16_to_f32(v);
        }
    if (bridge_transfer_fp16(net->w16, h.data(), P) || bridge_transfer_float32(net->master, m.data(), P)) {
        set_err(std::string("set_params: ") + (bridge_last_error() ? bridge_last_error() : ""));
        return -1;
    }
    bridge_gpu_memset(net->vel, 0, P * 4);
    net->wt_dirty = true;
    return net->fp8 && !quantise_weights(net, false) ? -1 : 0;
}

extern "C" int nnet_get_params(const KfNet *net, float *host) {
    if (!on_device(net, "get_params")) return -1;
    // D2H through the bridge (fp32 read = 2x fp16 count on a 4-byte aligned buffer)
    std::vector<uint16_t> tmp(net->nparams * 2);
    if (bridge_read_fp16(tmp.data(), net->master, net->nparams * 2)) {
        set_err("get_params");
        return -1;
    }
    memcpy(host, tmp.data(), net->nparams * 4);
    return 0;
}

// Replaces an idct-layer's fixed matrix (LoadWeights / allocWeightsFromKaldi, LayerIDCT:
// weight_loader.go:88-97, :760-770): host fp32 [dim x dim] in the y = x . M orientation,
// stored fp16 by truncation like every weight (tensor.go:158-173).
extern "C" int nnet_set_idct(KfNet *net, const char *layer, const float *m, int rows, int cols) {
    if (!on_device(net, "set_idct")) return -1;
    NetLayer *nl = find_layer(net, layer);
    if (!nl || nl->L.type != LayerType::IDCT || !nl->idct) {
        set_err(std::string("set_idct: no idct layer ") + (layer ? layer : "(null)"));
        return -1;
    }
    const int d = nl->L.out_dim;
    if (rows != d || cols != d || !m) {
        set_err("set_idct: " + nl->L.name + " needs a " + std::to_string(d) + "x" + std::to_string(d) +
                " matrix, got " + std::to_string(rows) + "x" + std::to_string(cols));
        return -1;
    }
    std::vector<uint16_t> h((size_t)d * d);
    for (size_t i = 0; i < h.size(); ++i) h[i] = f32_to_f16_trunc(m[i]);
    if (bridge_transfer_fp16(nl->idct, h.data(), h.size())) {
        set_err("set_idct: upload failed");
        return -1;
    }
    return 0;
}

// AttentionSpec.KeyScale from a loaded model (weight_loader.go:266-271)
extern "C" int nnet_set_key_scale(KfNet *net, const char *layer, float key_scale) {
    NetLayer *nl = find_layer(net, layer);
    if (nl && nl->L.type == LayerType::Attention && key_scale > 0) {
        nl->key_scale = key_scale;
        return 0;
    }
    set_err(std::string("set_key_scale: no attention layer ") + (layer ? layer : "(null)"));
    return -1;
}

extern "C" int nnet_set_bn(KfNet *net, const char *layer, int which, const float *mean,
                           const float *var, const float *gamma, const float *beta, float eps,
                           float target_rms) {
    if (!on_device(net, "set_bn")) return -1;
    auto no_bn = [&] {
        set_err(std::string("set_bn: no BatchNorm '") + std::to_string(which) + "' on layer " + layer);
        return -1;
    };
    NetLayer *nlp = find_layer(net, layer);
    if (!nlp) return no_bn();
    NetLayer &nl = *nlp;
    const Layer &L = nl.L;
    int dim, width;
    std::vector<float> *h;
    // target_rms <= 0: the layer's configured target-rms (batchnorm-component's, else 1)
    if (target_rms <= 0) target_rms = (which != 1 && L.type == LayerType::Batchnorm) ? (float)L.target_rms : 1.0f;
    if (which == 1) {
        if (L.type != LayerType::Prefinal) return no_bn();
        dim = width = L.small_dim;
        h = nl.hbn2;
        nl.bn2_eps = eps;
        nl.bn2_rms = target_rms;
    } else {
        if (L.type == LayerType::ConvReluBN) {
            dim = L.fout;
            width = L.out_dim;
        } else if (L.type == LayerType::Prefinal) {
            dim = width = L.big_dim;
        } else if (L.type == LayerType::TDNNF || L.type == LayerType::Batchnorm ||
                   L.type == LayerType::Attention) {
            dim = width = L.out_dim;
        } else {
            return no_bn();
        }
        h = nl.hbn;
        nl.bn_eps = eps;
        nl.bn_rms = target_rms;
    }
    h[0].assign(mean, mean + dim);
    h[1].assign(var, var + dim);
    h[2].assign(gamma, gamma + dim);
    h[3].assign(beta, beta + dim);
    if (which == 1) return upload_bn(net, h, eps, target_rms, dim, width, nl.bn2_scale, nl.bn2_shift) ? 0 : -1;
    return upload_bn(net, h, eps, target_rms, dim, width, nl.bn_scale, nl.bn_shift) ? 0 : -1;
}

extern "C" float *nnet_grad_buffer(KfNet *net) { return net->grad; }
extern "C" float *nnet_master_buffer(KfNet *net) { return net->master; }
extern "C" void *nnet_weight_buffer(KfNet *net) {
    net->wt_dirty = true;  // the caller may write the weights through it
    return net->w16;
}

// Parse + resolve only (no device work): one line per layer
// "name type in_dim out_dim" followed by "params N". Returns bytes needed, -1 on error.
extern "C" int nnet_parse_summary(const char *xconfig_text, char *out, int outlen) {
    std::vector<kf::LayerConfig> cfgs;
    std::vector<Layer> layers;
    std::string err;
    if (!kf::ParseXConfig(xconfig_text ? xconfig_text : "", cfgs, err) ||
        !kf::ResolveLayers(cfgs, layers, err)) {
        set_err("parse xconfig: " + err);
        return -1;
    }
    std::string s;
    long long nparams = 0;
    for (const Layer &L : layers) {
        s += L.name + " " + std::to_string((int)L.type) + " " + std::to_string(L.in_dim) + " " +
             std::to_string(L.out_dim) + "\n";
        switch (L.type) {
            case LayerType::ConvReluBN:
                nparams += (long long)L.time_offsets.size() * L.height_offsets.size() * L.fin * L.fout + L.fout;
                break;
            case LayerType::TDNNF: {
                int k = L.time_stride > 0 ? 2 : 1;
                nparams += (long long)k * L.in_dim * L.bottleneck + (long long)k * L.bottleneck * L.out_dim + L.out_dim;
                break;
            }
            case LayerType::Linear: nparams += (long long)L.in_dim * L.out_dim; break;
            case LayerType::Prefinal:
                nparams += (long long)L.in_dim * L.big_dim + L.big_dim + (long long)L.big_dim * L.small_dim;
                break;
            case LayerType::Output: nparams += (long long)L.in_dim * L.out_dim + L.out_dim; break;
            default: break;
        }
    }
    s += "params " + std::to_string(nparams) + "\n";
    if (out && outlen > 0) snprintf(out, outlen, "%s", s.c_str());
    return (int)s.size() + 1;
}
