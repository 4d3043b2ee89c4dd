// network.cpp — the network of the C++ host layer: topology, allocation, parameters and
// setters, MXFP8 set-up, SGD and the Kaldi-style update, the data-parallel plan (forward.cpp /
// backward.cpp: the passes).
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

static bool quantise_weights(KfNet *net, bool alloc);
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
    for (auto &nl : net->layers) {
        if (nl.L.name != layer) continue;
        if (nl.L.type != LayerType::IDCT || !nl.idct) break;
        const int d = nl.L.out_dim;
        if (rows != d || cols != d || !m) {
            set_err("set_idct: " + nl.L.name + " needs a " + std::to_string(d) + "x" + std::to_string(d) +
                    " matrix, got " + std::to_string(rows) + "x" + std::to_string(cols));
            return -1;
        }
        std::vector<uint16_t> h((size_t)d * d);
        for (size_t i = 0; i < h.size(); ++i) h[i] = f32_to_f16_trunc(m[i]);
        if (bridge_transfer_fp16(nl.idct, h.data(), h.size())) {
            set_err("set_idct: upload failed");
            return -1;
        }
        return 0;
    }
    set_err(std::string("set_idct: no idct layer ") + (layer ? layer : "(null)"));
    return -1;
}

// AttentionSpec.KeyScale from a loaded model (weight_loader.go:266-271)
extern "C" int nnet_set_key_scale(KfNet *net, const char *layer, float key_scale) {
    for (auto &nl : net->layers)
        if (nl.L.name == layer && nl.L.type == LayerType::Attention && key_scale > 0) {
            nl.key_scale = key_scale;
            return 0;
        }
    set_err(std::string("set_key_scale: no attention layer ") + (layer ? layer : "(null)"));
    return -1;
}

extern "C" int nnet_set_bn(KfNet *net, const char *layer, int which, const float *mean,
                           const float *var, const float *gamma, const float *beta, float eps,
                           float target_rms) {
    if (!on_device(net, "set_bn")) return -1;
    for (auto &nl : net->layers) {
        if (nl.L.name != layer) continue;
        const Layer &L = nl.L;
        int dim, width;
        std::vector<float> *h;
        // target_rms <= 0: the layer's configured target-rms (batchnorm-component's, else 1)
        if (target_rms <= 0) target_rms = (which != 1 && L.type == LayerType::Batchnorm) ? (float)L.target_rms : 1.0f;
        if (which == 1) {
            if (L.type != LayerType::Prefinal) break;
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
                break;
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
    set_err(std::string("set_bn: no BatchNorm '") + std::to_string(which) + "' on layer " + layer);
    return -1;
}

// ---------------------------------------------------------------------------
// MXFP8 forward (configs[4] of BASELINE.json: "OCP-FP8 MFMA GEMM path")
// Every dense GEMM of TDNN-F / linear / prefinal / output layers runs on
// v_mfma_scale_f32_16x16x128_f8f6f4 when its input has an MXFP8 copy; the
// copies are written by the producing GEMM's epilogue (out8), the weights are
// quantised after every parameter change. Widths are padded to 128 (zero
// elements, zero scale bytes), so splice parts stay whole K-steps.
// ---------------------------------------------------------------------------
namespace {
bool mx_alloc(KfNet *net, Mx &m, size_t rows, int width) {
    m.ld = pad128(width);
    m.q = (uint8_t *)net->dalloc(rows * m.ld + 64);
    m.s = (uint8_t *)net->dalloc(rows * (m.ld / 32) + 64);
    if (!m.q || !m.s) return false;
    bridge_gpu_memset(m.q, 0, rows * m.ld + 64);
    bridge_gpu_memset(m.s, 0, rows * (m.ld / 32) + 64);
    return true;
}
// W [nparts*rows x N] fp16 -> Mx [N x nparts*pad128(rows)]: one quantisation job per part
// (run together by quantise_weights)
bool mx_weights(KfNet *net, Mx &m, int pi, int nparts, int rows, int N, bool alloc,
                std::vector<KfQuantJob> &jobs) {
    const int part = pad128(rows);
    if (alloc) {
        m.ld = nparts * part;
        m.q = (uint8_t *)net->dalloc((size_t)N * m.ld + 64);
        m.s = (uint8_t *)net->dalloc((size_t)N * (m.ld / 32) + 64);
        if (!m.q || !m.s) return false;
    }
    const uint16_t *W = (const uint16_t *)wptr(net, pi);
    for (int p = 0; p < nparts; ++p)
        jobs.push_back(KfQuantJob{W + (size_t)p * rows * N, N, N, rows, 1, m.q + p * part, m.ld, m.s + p * part / 32,
                                  m.ld / 32});
    return true;
}
// W2 [2*bn x dout] -> w8d [bn x 2*pad128(dout)]: row j holds W2 rows j and bn + j, each
// quantised in 32-element blocks along dout (the reduction of the affine input gradient)
bool mx_dgrad_weights(KfNet *net, NetLayer &nl, bool alloc, std::vector<KfQuantJob> &jobs) {
    const int bn = nl.L.bottleneck, dout = nl.L.out_dim, part = pad128(dout);
    Mx &m = nl.w8d;
    if (alloc) {
        m.ld = 2 * part;
        m.q = (uint8_t *)net->dalloc((size_t)bn * m.ld + 64);
        m.s = (uint8_t *)net->dalloc((size_t)bn * (m.ld / 32) + 64);
        if (!m.q || !m.s) return false;
    }
    const uint16_t *W2 = (const uint16_t *)wptr(net, nl.pW2);
    for (int p = 0; p < 2; ++p)
        jobs.push_back(KfQuantJob{W2 + (size_t)p * bn * dout, dout, bn, dout, 0, m.q + p * part, m.ld,
                                  m.s + p * part / 32, m.ld / 32});
    return true;
}
// the layer's output can carry an MXFP8 copy (its epilogue has 32-column blocks)
bool f8_producer(const KfNet *net, int idx) {
    const NetLayer &nl = net->layers[idx];
    const Layer &L = nl.L;
    // conv: the epilogue's [(t,h) x fout] view must be the consumer's [t x hout*fout], and
    // only a non-conv consumer reads the copy (a conv's input is the fp16 halo image)
    if (L.type == LayerType::ConvReluBN) {
        bool mx_consumer = false;
        for (const auto &c : net->layers)
            mx_consumer = mx_consumer || (c.input == idx && c.L.type != LayerType::ConvReluBN);
        return mx_consumer && L.fin != 1 && L.fout % 32 == 0 && L.out_dim % 128 == 0;
    }
    return L.type == LayerType::TDNNF || L.type == LayerType::Linear ||
           (L.type == LayerType::Prefinal && L.small_dim % 32 == 0);
}
}  // namespace

// A consumer of a spec-augment layer that, in MXFP8 mode, reads the MXFP8 copy of the layer's
// input through the alias (net_internal.h in8): that copy is not masked. The consumer's name,
// or "" when there is none.
static std::string sa_mx_conflict(const KfNet *net) {
    for (const auto &c : net->layers) {
        if (c.input < 0 || net->layers[c.input].sa_ord < 0) continue;
        if (c.L.type != LayerType::TDNNF && c.L.type != LayerType::Linear && c.L.type != LayerType::Prefinal &&
            c.L.type != LayerType::Output)
            continue;
        int p = c.input;
        while (p >= 0 && net->layers[p].L.type == LayerType::SpecAugment) p = net->layers[p].input;
        if (p >= 0 && f8_producer(net, p)) return c.L.name;
    }
    return "";
}

static bool quantise_weights(KfNet *net, bool alloc) {
    std::vector<KfQuantJob> jobs;
    for (auto &nl : net->layers) {
        const Layer &L = nl.L;
        bool ok = true;
        switch (L.type) {
            case LayerType::TDNNF: {
                const int np = L.time_stride > 0 ? 2 : 1;
                ok = mx_weights(net, nl.w8, nl.pW, np, L.in_dim, L.bottleneck, alloc, jobs) &&
                     mx_weights(net, nl.w8b, nl.pW2, np, L.bottleneck, L.out_dim, alloc, jobs) &&
                     (np == 1 || mx_dgrad_weights(net, nl, alloc, jobs));
                break;
            }
            case LayerType::Linear:
            case LayerType::Output:
                ok = mx_weights(net, nl.w8, nl.pW, 1, L.in_dim, L.out_dim, alloc, jobs);
                break;
            case LayerType::Prefinal:
                ok = mx_weights(net, nl.w8, nl.pW, 1, L.in_dim, L.big_dim, alloc, jobs) &&
                     mx_weights(net, nl.w8b, nl.pW2, 1, L.big_dim, L.small_dim, alloc, jobs);
                break;
            default:
                break;
        }
        if (!ok) return false;
    }
    for (size_t j = 0; j < jobs.size(); j += KF_QUANT_MAX)
        if (!ck(kf_quant_mxfp8_batch((int)std::min<size_t>(KF_QUANT_MAX, jobs.size() - j), jobs.data() + j),
                "quantise weights"))
            return false;
    return true;
}

extern "C" int nnet_set_fp8(KfNet *net, int on) {
    kf_take_pending(__func__);
    if (!on_device(net, "set_fp8")) return -1;
    if (!on) {
        net->fp8 = 0;
        return 0;
    }
    if (net->ng_on) {
        set_err("set_fp8: not supported with natural gradient on (nnet_set_natural_gradient)");
        return -1;
    }
    if (drop_active(net)) {
        set_err("set_fp8: not supported with dropout on (nnet_set_dropout)");
        return -1;
    }
    if (bnt_active(net)) {
        set_err("set_fp8: not supported with training-mode BatchNorm on (nnet_set_bn_train)");
        return -1;
    }
    if (sa_active(net) && !sa_mx_conflict(net).empty()) {
        set_err("set_fp8: with SpecAugment on (nnet_set_spec_augment) layer " + sa_mx_conflict(net) +
                " would read the unmasked MXFP8 copy of a spec-augment layer's input");
        return -1;
    }
    net->fp8_dgrad = on != 2;
    if (!net->fp8) {
        const size_t T = (size_t)net->max_T;
        bool first = true;
        for (auto &nl : net->layers) first = first && !nl.w8.q;
        for (size_t i = 0; i < net->layers.size(); ++i) {
            NetLayer &nl = net->layers[i];
            const Layer &L = nl.L;
            if (first && f8_producer(net, (int)i) && !mx_alloc(net, nl.a8, T, L.out_dim)) {
                set_err("fp8: alloc " + L.name);
                return -1;
            }
            if (first && (L.type == LayerType::TDNNF || L.type == LayerType::Prefinal) &&
                !mx_alloc(net, nl.x8, T, L.type == LayerType::TDNNF ? L.bottleneck : L.big_dim)) {
                set_err("fp8: alloc " + L.name);
                return -1;
            }
        }
        // dz copies for the TDNN-F affine input gradients: as wide as the widest such layer
        int dzw = 0;
        for (auto &nl : net->layers)
            if (nl.L.type == LayerType::TDNNF && nl.L.time_stride > 0) dzw = std::max(dzw, nl.L.out_dim);
        for (int i = 0; first && dzw > 0 && i < 3; ++i)
            if (!mx_alloc(net, net->dz8[i], T, dzw)) {
                set_err("fp8: alloc dz copies");
                return -1;
            }
        if (!quantise_weights(net, first)) return -1;
    }
    net->fp8 = 1;
    return 0;
}

extern "C" int nnet_set_implicit_dz(KfNet *net, int on) {
    if (!net) return -1;
    if (on && drop_active(net)) {
        set_err("set_implicit_dz: not supported with dropout on (nnet_set_dropout)");
        return -1;
    }
    if (on && bnt_active(net)) {
        set_err("set_implicit_dz: not supported with training-mode BatchNorm on (nnet_set_bn_train)");
        return -1;
    }
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
    if (bnt_active(net)) {
        set_err("set_row_subsampling: not supported with training-mode BatchNorm on (nnet_set_bn_train)");
        return -1;
    }
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
    }
    net->rs_nt = nt;
    net->maxTc = maxTc;
    net->rsub = 3;
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

extern "C" int nnet_set_wgrad_stream(KfNet *net, int on) {
    if (!net) return -1;
    if (!on && net->wg_stream) bridge_gpu_sync();
    net->wg_side = on != 0 && net->wg_stream != nullptr;
    return 0;
}

extern "C" float *nnet_grad_buffer(KfNet *net) { return net->grad; }
extern "C" float *nnet_master_buffer(KfNet *net) { return net->master; }
extern "C" void *nnet_weight_buffer(KfNet *net) {
    net->wt_dirty = true;  // the caller may write the weights through it
    return net->w16;
}

extern "C" int nnet_weights_changed(KfNet *net) {
    if (!on_device(net, "weights_changed")) return -1;
    net->wt_dirty = true;  // the transposed copies are refreshed at the next forward
    return net->fp8 && !quantise_weights(net, false) ? -1 : 0;
}

extern "C" int nnet_sgd(KfNet *net, float lr, float momentum) {
    kf_take_pending(__func__);
    if (!on_device(net, "sgd")) return -1;
    if (!ck(kf_sgd_flat(net->master, net->w16, net->grad, net->vel, lr, momentum, net->nparams), "sgd"))
        return -1;
    net->wt_dirty = true;
    // the MXFP8 weight copies follow every parameter change
    return net->fp8 && !quantise_weights(net, false) ? -1 : 0;
}

// ---------------------------------------------------------------------------
// Kaldi-style update (kf_nnet.h nnet_update): per-component max-change, L2 and
// learning-rate factor over the flat buffers, one kf_update_maxchange call per step
// ---------------------------------------------------------------------------
// The two kernels' entry points are weak references: a program that links the host layer
// against a backend without them (the tests' launch-trace stub) still links, and
// nnet_update reports them missing.
#pragma weak kf_update_maxchange
#pragma weak kf_update_scratch_bytes

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
    if (!ck(kf_update_maxchange(net->master, net->w16, net->grad, net->vel, net->nparams,
                                (const KfUpdSegment *)net->upd_segs, net->upd_nseg, (const KfUpdComp *)net->upd_comps,
                                (int)net->comps.size(), lr, momentum, max_param_change, l2_scale, net->upd_scratch,
                                net->upd_stats),
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
// Semi-orthogonal constraint (kf_nnet.h nnet_constrain_orthonormal): Kaldi's
// ConstrainOrthonormal over every constrained component, one kf_orthonormal_constrain call
// ---------------------------------------------------------------------------
// weak, as the update's entry points above: the launch-trace stub backend has neither
#pragma weak kf_orthonormal_constrain
#pragma weak kf_orthonormal_scratch_bytes

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
    for (int i = 0; i < n && i < (int)v.size(); ++i)
        if (idx) idx[i] = v[i];
    return (int)v.size();
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

// ---------------------------------------------------------------------------
// Natural-gradient preconditioning (kf_nnet.h nnet_set_natural_gradient): the
// tables and buffers; nnet_backward (backward.cpp) issues the statistics and the launches
// ---------------------------------------------------------------------------
// weak, as the update's entry points above: the launch-trace stub backend has none of them
#pragma weak kf_ng_init
#pragma weak kf_ng_default_opts
#pragma weak kf_ng_apply_scratch_bytes
#pragma weak kf_ng_state_scratch_bytes

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
    if (net->fp8) {
        set_err("set_natural_gradient: not supported in MXFP8 mode (nnet_set_fp8)");
        return -1;
    }
    if (net->dp) {
        set_err("set_natural_gradient: not supported on a net bound to data parallel (nnet_bind_dp)");
        return -1;
    }
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
    if (net->ng_on) {
        set_err("bind_dp: not supported with natural gradient on (nnet_set_natural_gradient)");
        return -1;
    }
    if (bnt_active(net)) {
        set_err("bind_dp: not supported with training-mode BatchNorm on (nnet_set_bn_train): the statistics "
                "would be each rank's own");
        return -1;
    }
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
    if (!net) return -1;
    for (int i = 0; idx && i < n && i < (int)net->drop_layers.size(); ++i) idx[i] = net->drop_layers[i];
    return (int)net->drop_layers.size();
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
    for (auto &nl : net->layers)
        if (nl.L.name == layer) {
            if (nl.drop_ord < 0) {
                set_err(std::string("set_dropout_proportion: layer ") + layer + " has no dropout component");
                return -1;
            }
            nl.drop_p = p;
            return 0;
        }
    set_err(std::string("set_dropout_proportion: no layer ") + layer);
    return -1;
}

extern "C" int nnet_dropout_proportion(const KfNet *net, const char *layer, float *p) {
    if (net && layer)
        for (const auto &nl : net->layers)
            if (nl.L.name == layer) {
                if (p) *p = nl.drop_ord < 0 ? -1.f : nl.drop_p;
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
        if (net->fp8 || net->implicit_dz) {
            set_err("set_dropout: not supported in MXFP8 mode (nnet_set_fp8) or with implicit dz (nnet_set_implicit_dz)");
            return -1;
        }
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
    for (auto &nl : net->layers) {
        if (!layer || nl.L.name != layer) continue;
        if (nl.drop_ord < 0 || !nl.drop_act || !nl.drop) {
            set_err(std::string("dropout_mask: the last forward drew no mask for ") + layer +
                    (nl.drop_ord < 0 ? " (no dropout component)" : " (dropout off or proportion 0)"));
            return -1;
        }
        if (B) *B = net->drop_B;
        if (dim) *dim = nl.L.out_dim;
        // (ordered behind the forward on the current stream, and synchronises; fp32 read = 2x
        // fp16 count, as nnet_update_stats)
        if (host && bridge_read_fp16((uint16_t *)host, nl.drop, (size_t)net->drop_B * nl.L.out_dim * 2)) {
            set_err("dropout_mask: read");
            return -1;
        }
        return 0;
    }
    set_err(std::string("dropout_mask: no layer ") + (layer ? layer : "(null)"));
    return -1;
}

// ---------------------------------------------------------------------------
// SpecAugment of the spec-augment layers (kf_nnet.h nnet_set_spec_augment): the
// switch, the options and the step. forward.cpp draws and applies the masks.
// ---------------------------------------------------------------------------
static NetLayer *sa_layer(KfNet *net, const char *layer, const char *what) {
    if (net && layer)
        for (auto &nl : net->layers)
            if (nl.L.name == layer) {
                if (nl.sa_ord >= 0) return &nl;
                set_err(std::string(what) + ": layer " + layer + " is not a spec-augment-layer");
                return nullptr;
            }
    set_err(std::string(what) + ": no layer " + (layer ? layer : "(null)"));
    return nullptr;
}

extern "C" int nnet_spec_augment_layers(const KfNet *net, int *idx, int n) {
    if (!net) return -1;
    for (int i = 0; idx && i < n && i < (int)net->sa_layers.size(); ++i) idx[i] = net->sa_layers[i];
    return (int)net->sa_layers.size();
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
    if (on && net->fp8 && !net->sa_layers.empty() && !sa_mx_conflict(net).empty()) {
        set_err("set_spec_augment: in MXFP8 mode (nnet_set_fp8) layer " + sa_mx_conflict(net) +
                " would read the unmasked MXFP8 copy of a spec-augment layer's input");
        return -1;
    }
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
#pragma weak kf_bn_train_stats

static NetLayer *bnt_layer(KfNet *net, const char *layer, int which, const char *what) {
    if (net && layer)
        for (int li : net->bnt_layers)
            if (net->layers[li].L.name == layer && which == 0) return &net->layers[li];
    set_err(std::string(what) + ": training-mode BatchNorm (nnet_set_bn_train) does not govern BatchNorm '" +
            std::to_string(which) + "' of layer " + (layer ? layer : "(null)"));
    return nullptr;
}

extern "C" int nnet_bn_train_layers(const KfNet *net, int *idx, int n) {
    if (!net) return -1;
    for (int i = 0; idx && i < n && i < (int)net->bnt_layers.size(); ++i) idx[i] = net->bnt_layers[i];
    return (int)net->bnt_layers.size();
}

extern "C" int nnet_set_bn_train(KfNet *net, int on) {
    if (!on_device(net, "set_bn_train")) return -1;
    if (!on || net->bnt_layers.empty()) {
        net->bnt_on = on != 0;
        return 0;
    }
    if (net->fp8) {
        set_err("set_bn_train: not supported in MXFP8 mode (nnet_set_fp8)");
        return -1;
    }
    if (net->implicit_dz) {
        set_err("set_bn_train: not supported with implicit dz (nnet_set_implicit_dz)");
        return -1;
    }
    if (net->rsub) {
        // (the compact row set's scratch row and inexact tail rows are not rows of the layer)
        set_err("set_bn_train: not supported with row subsampling (nnet_set_row_subsampling)");
        return -1;
    }
    if (net->dp) {
        set_err("set_bn_train: not supported with a data-parallel communicator bound (nnet_bind_dp): the statistics "
                "would be each rank's own");
        return -1;
    }
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
