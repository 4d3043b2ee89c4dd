// mxfp8.cpp — the MXFP8 mode of the host layer (nnet_set_fp8): the copies' storage and the
// weight quantisation that follows every parameter change.
#include "net_internal.h"

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
// input through the alias (net_internal.h in8): that copy is not masked. What an error says of
// it (the mode-conflict table's condition, modes.cpp), or "" when there is none.
std::string sa_mx_conflict(const KfNet *net) {
    for (const auto &c : net->layers) {
        if (c.input < 0 || net->layers[c.input].sa_ord < 0) continue;
        if (c.L.type != LayerType::TDNNF && c.L.type != LayerType::Linear && c.L.type != LayerType::Prefinal &&
            c.L.type != LayerType::Output)
            continue;
        int p = c.input;
        while (p >= 0 && net->layers[p].L.type == LayerType::SpecAugment) p = net->layers[p].input;
        if (p >= 0 && f8_producer(net, p))
            return "layer " + c.L.name + " would read the unmasked MXFP8 copy of a spec-augment layer's input";
    }
    return "";
}

bool quantise_weights(KfNet *net, bool alloc) {
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
    if (!admit(net, Mode::Fp8, "set_fp8")) return -1;
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

extern "C" int nnet_weights_changed(KfNet *net) {
    if (!on_device(net, "weights_changed")) return -1;
    net->wt_dirty = true;  // the transposed copies are refreshed at the next forward
    return net->fp8 && !quantise_weights(net, false) ? -1 : 0;
}
