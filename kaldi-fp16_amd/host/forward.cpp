// forward.cpp — the forward pass of the C++ host layer (Network.Forward, forward.go:148-202,
// and the per-layer forward functions): one function per layer kind, each a few fused
// launches (network.cpp's header comment).
#include <cmath>

#include "net_internal.h"

namespace {

// k-contiguous (transposed) copies of the short-K forward weights: the tiled GEMM's
// k-contiguous B path beats its reduction-major one on these shapes (TDNN-F affine
// forward with the full epilogue 243 -> 225 us, DESIGN.md §7 performance log, r2)
bool refresh_wt(KfNet *net) {
    if (!net->wt_dirty) return true;
    // one launch for every layer's copy (was one ops_transpose each: 18 x 9 us per step)
    std::vector<const void *> src;
    std::vector<void *> dst;
    std::vector<int> M, N;
    auto flush = [&]() {
        const bool ok = src.empty() || ck(kf_transpose_batch((int)src.size(), src.data(), dst.data(), M.data(),
                                                             N.data()),
                                          "transpose weights");
        src.clear(), dst.clear(), M.clear(), N.clear();
        return ok;
    };
    for (auto &nl : net->layers) {
        if (!nl.wt) continue;
        src.push_back(wptr(net, nl.wt_pi));
        dst.push_back(nl.wt);
        M.push_back(nl.wt_K);
        N.push_back(nl.wt_N);
        if ((int)src.size() == KF_TRANSPOSE_MAX && !flush()) return false;
    }
    if (!flush()) return false;
    net->wt_dirty = false;
    return true;
}

// relu + BatchNorm epilogue into the layer's activation / mask (conv, TDNN-F affine)
KfEpilogue epi_relu_bn(KfNet *net, NetLayer &nl, int pb, long long ldo) {
    KfEpilogue E = epi0();
    E.out = nl.act;
    E.ldo = ldo;
    E.bias = wptr(net, pb);
    E.relu = 1;
    E.mask_out = nl.mask;
    E.scale = nl.bn_scale;
    E.shift = nl.bn_shift;
    return E;
}

// Training-mode BatchNorm of a governed site: the batch statistics of r [rows x H F]
// (block f = column h F + f; H = 1: the column entries), then r scale + shift into out through the
// dense [rows H x F] view. stat = mean | var | scale | shift, acc = count (2) | sum | sumsq.
// The statistics run over the first stat_rows rows, the apply over all `rows` (a
// compact layer's rows c < Tc0 against its Tc; everywhere else the two are equal).
// relu (self-repair, DESIGN §31: count (2) | deriv_sum, or NULL): the same pass counts the active units.
bool bnt_normalise(const void *r, int stat_rows, int rows, int H, int F, float eps, float rms, float *stat, double *acc,
                   void *out, const std::string &what, double *relu = nullptr) {
    // (H = 1, a prefinal layer or a batchnorm-component: wide rows, the column entry's lane map)
    int rc;
    if (relu)
        rc = H == 1 ? kf_bn_train_stats_relu(r, F, stat_rows, F, eps, rms, stat, stat + F, stat + 2 * F, stat + 3 * F, acc,
                                             acc + 2, acc + 2 + F, relu, relu + 2)
                    : kf_bn_block_stats_relu(r, (long long)H * F, stat_rows, H, F, eps, rms, stat, stat + F, stat + 2 * F,
                                             stat + 3 * F, acc, acc + 2, acc + 2 + F, relu, relu + 2);
    else
        rc = H == 1 ? kf_bn_train_stats(r, F, stat_rows, F, eps, rms, stat, stat + F, stat + 2 * F, stat + 3 * F, acc, acc + 2,
                                        acc + 2 + F)
                    : kf_bn_block_stats(r, (long long)H * F, stat_rows, H, F, eps, rms, stat, stat + F, stat + 2 * F,
                                        stat + 3 * F, acc, acc + 2, acc + 2 + F);
    return ck(rc, (what + " batchnorm statistics").c_str()) &&
           ck(kf_bn_train_apply(r, F, rows * H, F, stat + 2 * F, stat + 3 * F, nullptr, 0, nullptr, nullptr, 0, 0.f, out, F),
              (what + " batchnorm apply").c_str());
}
bool bnt_conv(NetLayer &nl, int T) {
    return bnt_normalise(nl.bnt_r, T, T, nl.L.hout, nl.L.fout, nl.bn_eps, nl.bn_rms, nl.bnt_stat, nl.bnt_acc, nl.act, "conv",
                         nl.sr_act ? nl.sr_acc : nullptr);
}
// the epilogue of a governed conv / prefinal affine: r and the ReLU mask, no scale or shift
KfEpilogue epi_relu_r(KfNet *net, NetLayer &nl, int pb, long long ldo) {
    KfEpilogue E = epi_relu_bn(net, nl, pb, ldo);
    E.out = nl.bnt_r;
    E.scale = E.shift = nullptr;
    return E;
}

bool fwd_combine(KfNet *net, NetLayer &nl, const void *x, int T) {
    const Layer &L = nl.L;
    if (nl.input2 != -100) {  // Append(a, b): b broadcast per sequence when per_seq
        const bool bseq = nl.input2 == -2 || (nl.input2 >= 0 && net->layers[nl.input2].per_seq);
        return ck(kf_combine_feature_maps(x, L.height * L.nf1, act_of(net, nl.input2), L.height * L.nf2,
                                          bseq ? net->seq_off : nullptr, net->B, nl.act, L.out_dim, T, L.height,
                                          L.nf1, L.nf2),
                  "combine");
    }
    return ck(ops_copy(nl.act, x, T * L.out_dim), "combine copy") &&
           ck(ops_combine_feature_maps(nl.act, T, L.out_dim, L.height, L.nf1, L.nf2), "combine");
}

// small fin (Kaldi's cnn1 after combine-feature-maps: 6): im2col + GEMM
bool fwd_conv_small_fin(KfNet *net, NetLayer &nl, const void *x, int T) {
    const Layer &L = nl.L;
    const int K = (int)nl.dt.size() * L.fin;
    if (!ck(kf_im2col_small(x, L.in_dim, T, L.hin, L.hout, L.hsub, L.fin, (int)nl.dt.size(), nl.dt.data(),
                            nl.dh.data(), nl.im2col, nl.kp),
            "im2col small") ||
        !ck(ops_copy(nl.wpad, wptr(net, nl.pW), K * L.fout), "conv weight pad"))
        return false;
    KfOperand A = op_base(nl.im2col, nl.kp, T * L.hout, nl.kp, 1);
    KfOperand B = op_base(nl.wpad, L.fout, nl.kp, L.fout, 0);
    KfEpilogue E = nl.bnt_act ? epi_relu_r(net, nl, nl.pb, L.fout) : epi_relu_bn(net, nl, nl.pb, L.fout);
    return ck(kf_gemm_fused(T * L.hout, L.fout, nl.kp, &A, &B, &E), "conv small fin") && (!nl.bnt_act || bnt_conv(nl, T));
}

// The conv below the compact layers on the compact rows: output frames 3c (c < Tc0), and
// the tail tail_t0 ... T-1 (compact rows Tc0 ..): two time-strided launches into compact
// rows. The tail's few workgroups (latency: the whole K loop for ~200 rows) run beside the
// main launch on the weight-gradient stream.
bool fwd_conv_compact(KfNet *net, NetLayer &nl, int K, KfOperand A, const KfOperand &B, const KfEpilogue &E) {
    const Layer &L = nl.L;
    const RowSet &rs = net->rs;
    void *const cst = kf_get_stream();
    const bool side = rs.nt > 0 && net->wg_stream;
    if (rs.nt > 0) {
        const size_t r0 = (size_t)rs.Tc0 * L.hout * L.fout;  // elements
        KfOperand At = A;
        At.tmul = 3;
        At.t0 = rs.tail_t0;
        At.nrows = rs.nt * L.hout;
        KfEpilogue Et = E;
        Et.out = (char *)nl.act + r0 * 2;
        Et.mask_out = nl.mask + r0 / 8;
        auto tail = [&] { return ck(kf_gemm_fused(rs.nt * L.hout, L.fout, K, &At, &B, &Et), "conv (compact tail rows)"); };
        if (side && (kf_event_record(net->ev_go, cst) != 0 || kf_stream_wait(net->wg_stream, net->ev_go) != 0)) {
            set_err("forward: conv tail stream order");
            return false;
        }
        if (side) kf_set_stream(net->wg_stream);
        const bool ok = side ? side_launch(net, cst, "forward: conv tail", tail) : tail();
        if (!side) kf_set_stream(cst);
        if (!ok) return false;
    }
    A.tmul = 3;
    A.nrows = rs.Tc0 * L.hout;
    if (!ck(kf_gemm_fused(rs.Tc0 * L.hout, L.fout, K, &A, &B, &E), "conv (compact rows)")) return false;
    return !side || aux_join(net, cst, "forward: conv tail");
}

bool fwd_conv(KfNet *net, int li, const void *x, int T) {
    NetLayer &nl = net->layers[li];
    const Layer &L = nl.L;
    if (L.fin == 1 && nl.bnt_act)  // (no scale: the kernel stores r = relu(conv + bias))
        return ck(kf_conv_c1_forward(T, L.hin, L.hout, L.hsub, L.fout, (int)nl.dt.size(), nl.dt.data(), nl.dh.data(), x,
                                     wptr(net, nl.pW), wptr(net, nl.pb), nullptr, nullptr, nl.bnt_r, nl.mask),
                  "conv c1") &&
               bnt_conv(nl, T);
    if (L.fin == 1)
        return ck(kf_conv_c1_forward(T, L.hin, L.hout, L.hsub, L.fout, (int)nl.dt.size(), nl.dt.data(), nl.dh.data(), x,
                                     wptr(net, nl.pW), wptr(net, nl.pb), nl.bn_scale, nl.bn_shift, nl.act, nl.mask),
                  "conv c1");
    if (nl.kp) return fwd_conv_small_fin(net, nl, x, T);
    const int K = (int)nl.dt.size() * L.fin;
    KfOperand A = op_im2col(nl, x, T, 1);
    KfOperand B = op_base(wptr(net, nl.pW), L.fout, K, L.fout, 0);
    KfEpilogue E = epi_relu_bn(net, nl, nl.pb, L.fout);
    if (net->fp8 && nl.a8.q) set_out8(E, nl.a8), E.ldo8 = L.fout;  // rows (t,h) of fout: the [t x hout*fout] copy
    if (conv_compact(net, li)) return fwd_conv_compact(net, nl, K, A, B, E);
    // (MXFP8 is refused with the mode and a governed conv below the row set runs on full rows,
    // conv_c_on: no out8, no compact rows)
    if (nl.bnt_act) {
        KfEpilogue Er = epi_relu_r(net, nl, nl.pb, L.fout);
        return ck(kf_gemm_fused(T * L.hout, L.fout, K, &A, &B, &Er), "conv") && bnt_conv(nl, T);
    }
    return ck(kf_gemm_fused(T * L.hout, L.fout, K, &A, &B, &E), "conv");
}

bool fwd_tdnnf(KfNet *net, int li, const void *x) {
    NetLayer &nl = net->layers[li];
    const Layer &L = nl.L;
    const int T = rows_of(net, li);  // compact rows
    const int din = L.in_dim, dout = L.out_dim;
    const int s = nl.compact && net->rs.Tc ? L.time_stride / 3 : L.time_stride, bn = L.bottleneck;
    const int klin = s > 0 ? 2 * din : din, kaff = s > 0 ? 2 * bn : bn;
    const int np = s > 0 ? 2 : 1;
    const Mx *x8 = in8(net, nl);
    KfOperand A = x8 ? op_mx(*x8, T, np, -s, 0)
                     : s > 0 ? op_splice(x, T, din, -s, 0, KF_CLAMP, 1) : op_base(x, din, T, din, 1);
    // compact rows with a tail: row Tc0 - 1's +1 neighbour in the affine splice is row
    // T-1 (the tail's last row). The scratch row Tc0 reads the last row's linear inputs
    // [x(Tc-1-s) | x(Tc-1)] (edge rows), so its bottleneck is that row's, bit for bit
    // (nnet_set_row_subsampling)
    const bool scratch = nl.compact && net->rs.Tc > net->rs.Tc0 && s > 0;
    if (scratch && !x8) {
        A.edge_t[0] = A.edge_t[1] = net->rs.Tc0;
        A.edge_row[0] = std::max(0, net->rs.Tc - 1 - s);
        A.edge_row[1] = net->rs.Tc - 1;
    }
    KfOperand B = x8 ? op_mxw(nl.w8, bn) : op_base(wptr(net, nl.pW), bn, klin, bn, 0);
    KfEpilogue E = epi0();
    E.out = nl.aux;
    E.ldo = bn;
    // the bottleneck's MXFP8 copy is quantised after the GEMM rather than in its
    // epilogue: out8 needs 32-column blocks inside one wave's tile, which would
    // force 256x256 tiles onto N = bottleneck (320 of 512 columns used) instead of
    // 384x160 (3072 model: 331 -> see DESIGN §7)
    if (!ck(kf_gemm_fused(T, bn, x8 ? nl.w8.ld : klin, &A, &B, &E), "tdnnf linear")) return false;
    if (scratch && x8 &&
        !ck(ops_copy((char *)nl.aux + (size_t)net->rs.Tc0 * bn * 2,
                     (const char *)nl.aux + (size_t)(net->rs.Tc - 1) * bn * 2, bn),
            "row set edge copy"))
        return false;
    const bool f8b = net->fp8 && nl.x8.q;
    if (f8b && !ck(kf_quant_mxfp8(nl.aux, bn, T, bn, 0, nl.x8.q, nl.x8.ld, nl.x8.s, nl.x8.ld / 32), "quantise bottleneck"))
        return false;
    KfOperand A2 = f8b ? op_mx(nl.x8, T, np, 0, s)
                       : s > 0 ? op_splice(nl.aux, T, bn, 0, s, KF_CLAMP, 1) : op_base(nl.aux, bn, T, bn, 1);
    KfOperand B2 = f8b     ? op_mxw(nl.w8b, dout)
                   : nl.wt ? op_base(nl.wt, kaff, dout, kaff, 1)
                           : op_base(wptr(net, nl.pW2), dout, kaff, dout, 0);
    KfEpilogue E2 = epi_relu_bn(net, nl, nl.pb2, dout);
    if (net->fp8) set_out8(E2, nl.a8);
    if (nl.bypass) {
        E2.resid = x;
        E2.ldr = din;
        E2.resid_alpha = (float)L.bypass_scale;
    }
    if (nl.drop_act) {  // relu -> batchnorm -> dropout -> + bypass (the bypass is not masked)
        E2.drop = nl.drop;
        E2.ld_drop = dout;
        E2.row_seg = drop_rows(net, nl.compact);
    }
    if (!nl.bnt_act) return ck(kf_gemm_fused(T, dout, f8b ? nl.w8b.ld : kaff, &A2, &B2, &E2), "tdnnf affine");
    // training-mode BatchNorm: the GEMM writes r = relu(affine + bias) and the mask
    // only; the batch statistics of r, then the epilogue's scale / shift / dropout / bypass on them.
    // On compact rows the statistics are those of the rows c < Tc0, applied to all Tc.
    KfEpilogue Er = epi_relu_bn(net, nl, nl.pb2, dout);
    Er.out = nl.bnt_r;
    Er.scale = Er.shift = nullptr;
    float *const st = nl.bnt_stat;
    // (self-repair, DESIGN §31: the counting entry on the same pass)
    const int rc_gemm = kf_gemm_fused(T, dout, kaff, &A2, &B2, &Er);
    if (!ck(rc_gemm, "tdnnf affine")) return false;
    const int rc_stat =
        nl.sr_act ? kf_bn_train_stats_relu(nl.bnt_r, dout, bnt_stat_rows(net, li), dout, nl.bn_eps, nl.bn_rms, st, st + dout,
                                           st + 2 * dout, st + 3 * dout, nl.bnt_acc, nl.bnt_acc + 2, nl.bnt_acc + 2 + dout,
                                           nl.sr_acc, nl.sr_acc + 2)
                  : kf_bn_train_stats(nl.bnt_r, dout, bnt_stat_rows(net, li), dout, nl.bn_eps, nl.bn_rms, st, st + dout,
                                      st + 2 * dout, st + 3 * dout, nl.bnt_acc, nl.bnt_acc + 2, nl.bnt_acc + 2 + dout);
    return ck(rc_stat, "tdnnf batchnorm statistics") &&
           ck(kf_bn_train_apply(nl.bnt_r, dout, T, dout, st + 2 * dout, st + 3 * dout, E2.drop, E2.ld_drop, E2.row_seg,
                                E2.resid, E2.ldr, E2.resid_alpha, nl.act, dout),
              "tdnnf batchnorm apply");
}

// a plain x . W layer (linear, output): MXFP8 when the input has a copy
bool fwd_dense(KfNet *net, NetLayer &nl, const void *x, int T, int pb, const char *what) {
    const int din = nl.L.in_dim, dout = nl.L.out_dim;
    const Mx *x8 = in8(net, nl);
    KfOperand A = x8 ? op_mx(*x8, T, 1, 0, 0) : op_base(x, din, T, din, 1);
    KfOperand B = x8 ? op_mxw(nl.w8, dout) : op_base(wptr(net, nl.pW), dout, din, dout, 0);
    KfEpilogue E = epi0();
    E.out = nl.act;
    E.ldo = dout;
    E.bias = wptr(net, pb);
    if (net->fp8 && nl.L.type == LayerType::Linear) set_out8(E, nl.a8);
    return ck(kf_gemm_fused(T, dout, x8 ? nl.w8.ld : din, &A, &B, &E), what);
}

bool fwd_linear(KfNet *net, int li, const void *x) {
    NetLayer &nl = net->layers[li];
    const Layer &L = nl.L;
    if (nl.per_seq)  // ReplaceIndex branch: one row per sequence, any dims (ivector 100)
        return ck(kf_rows_gemm(x, L.in_dim, wptr(net, nl.pW), L.out_dim, nl.act, L.out_dim, net->B, L.in_dim, L.out_dim),
                  "ivector linear");
    return fwd_dense(net, nl, x, rows_of(net, li), -1, "linear");
}

// affine on the GPU (forward.go:813-826), then the per-head attention with
// ReLU + BatchNorm fused (the reference's CPU loop, :850-908)
bool fwd_attention(KfNet *net, NetLayer &nl, const void *x, int T) {
    const Layer &L = nl.L;
    const int A = att_affine(L), din = L.in_dim;
    KfOperand Aop = op_base(x, din, T, din, 1);
    KfOperand B = op_base(wptr(net, nl.pW), A, din, A, 0);
    KfEpilogue E = epi0();
    E.out = nl.aux;
    E.ldo = A;
    E.bias = wptr(net, nl.pb);
    if (!ck(kf_gemm_fused(T, A, din, &Aop, &B, &E), "attention affine")) return false;
    KfAttention att = att_args(nl, T);
    return ck(kf_attention_forward(&att, nl.act, L.out_dim, nl.mask, nl.bn_scale, nl.bn_shift), "attention");
}

bool fwd_prefinal(KfNet *net, int li, const void *x) {
    NetLayer &nl = net->layers[li];
    const Layer &L = nl.L;
    const int T = rows_of(net, li);
    const int din = L.in_dim, big = L.big_dim, small = L.small_dim;
    const Mx *x8 = in8(net, nl);
    KfOperand A = x8 ? op_mx(*x8, T, 1, 0, 0) : op_base(x, din, T, din, 1);
    KfOperand B = x8      ? op_mxw(nl.w8, big)
                  : nl.wt ? op_base(nl.wt, din, big, din, 1)
                          : op_base(wptr(net, nl.pW), big, din, big, 0);
    if (nl.bnt_act) {
        // training-mode BatchNorm: r_big -> statistics -> aux, then the linear output
        // r_small -> statistics -> act (no BatchNorm 1: the linear output is the activation)
        KfEpilogue Er = epi_relu_r(net, nl, nl.pb, big);
        KfOperand A2 = op_base(nl.aux, big, T, big, 1);
        KfOperand B2 = op_base(wptr(net, nl.pW2), small, big, small, 0);
        KfEpilogue E2 = epi0();
        E2.out = nl.has_bn2 ? nl.bnt_r2 : nl.act;
        E2.ldo = small;
        const int Ts = bnt_stat_rows(net, li);
        return ck(kf_gemm_fused(T, big, din, &A, &B, &Er), "prefinal big") &&
               bnt_normalise(nl.bnt_r, Ts, T, 1, big, nl.bn_eps, nl.bn_rms, nl.bnt_stat, nl.bnt_acc, nl.aux, "prefinal big",
                             nl.sr_act ? nl.sr_acc : nullptr) &&
               ck(kf_gemm_fused(T, small, big, &A2, &B2, &E2), "prefinal small") &&
               (!nl.has_bn2 || bnt_normalise(nl.bnt_r2, Ts, T, 1, small, nl.bn2_eps, nl.bn2_rms, nl.bnt_stat2, nl.bnt_acc2,
                                             nl.act, "prefinal small"));
    }
    KfEpilogue E = epi_relu_bn(net, nl, nl.pb, big);
    E.out = nl.aux;
    if (net->fp8) set_out8(E, nl.x8);
    if (!ck(kf_gemm_fused(T, big, x8 ? nl.w8.ld : din, &A, &B, &E), "prefinal big")) return false;
    const bool f8b = net->fp8 && nl.x8.q;
    KfOperand A2 = f8b ? op_mx(nl.x8, T, 1, 0, 0) : op_base(nl.aux, big, T, big, 1);
    KfOperand B2 = f8b ? op_mxw(nl.w8b, small) : op_base(wptr(net, nl.pW2), small, big, small, 0);
    KfEpilogue E2 = epi0();
    if (net->fp8) set_out8(E2, nl.a8);
    E2.out = nl.act;
    E2.ldo = small;
    if (nl.has_bn2) {
        E2.scale = nl.bn2_scale;
        E2.shift = nl.bn2_shift;
    }
    return ck(kf_gemm_fused(T, small, f8b ? nl.w8b.ld : big, &A2, &B2, &E2), "prefinal small");
}

bool fwd_layer(KfNet *net, int li, const void *x, int T) {
    NetLayer &nl = net->layers[li];
    const Layer &L = nl.L;
    switch (L.type) {
        case LayerType::IDCT:
            return ck(kf_small_gemm(x, L.in_dim, nl.idct, nl.act, L.out_dim, T, L.in_dim, L.out_dim), "idct");
        case LayerType::Batchnorm:
            if (nl.bnt_act)  // (the statistics of the input itself; a per-sequence layer's rows are the sequences)
                return bnt_normalise(x, nl.per_seq ? net->B : T, nl.per_seq ? net->B : T, 1, L.out_dim, nl.bn_eps, nl.bn_rms,
                                     nl.bnt_stat, nl.bnt_acc, nl.act, "batchnorm");
            return ck(kf_bn_apply(x, nl.act, nl.per_seq ? net->B : T, L.out_dim, nl.bn_scale, nl.bn_shift), "batchnorm");
        case LayerType::SpecAugment:
            // inactive: the alias of its input (forward.go:225-231 passes through). Active: the
            // select by the row_band sa_prepare drew, into the layer's own activation
            return !nl.sa_act ||
                   ck(kf_specaug_apply(x, L.in_dim, nl.act, L.out_dim, T, L.out_dim, nl.sa_rows), "spec-augment apply");
        case LayerType::CombineFeatureMaps: return fwd_combine(net, nl, x, T);
        case LayerType::ConvReluBN: return fwd_conv(net, li, x, T);
        case LayerType::TDNNF: return fwd_tdnnf(net, li, x);
        case LayerType::Linear: return fwd_linear(net, li, x);
        case LayerType::Attention: return fwd_attention(net, nl, x, T);
        case LayerType::Prefinal: return fwd_prefinal(net, li, x);
        case LayerType::Output: {
            const int Tl = rows_of(net, li);
            return fwd_dense(net, nl, x, Tl, nl.pb, "output") &&
                   (!L.include_log_softmax || ck(ops_log_softmax(nl.act, Tl, L.out_dim), "log_softmax"));
        }
        default:
            set_err("forward: unsupported layer " + L.name);
            return false;
    }
}

// Per-sequence dropout of this forward: the masks of every layer with a
// proportion > 0 in one launch, and the row -> sequence maps of the forward's row sets. The
// step advances at every forward while the switch is on, masks drawn or not. Storage is made
// at the first such forward and again only when a forward brings more sequences than any
// before it: nothing is allocated per step.
bool drop_prepare(KfNet *net) {
    net->drop_live = false;
    for (int li : net->drop_layers) net->layers[li].drop_act = false;
    if (!drop_active(net)) return true;
    if (!admit(net, Mode::Dropout, "forward")) return false;  // (the setters' rule, where the forward would break it)
    const long long step = net->drop_step;
    net->drop_step = (step + 1) & 0xFFFFFFFFll;
    std::vector<KfDropLayer> tab;
    for (int li : net->drop_layers)
        if (net->layers[li].drop_p > 0.f) tab.push_back(KfDropLayer{nullptr, 0, 0, 0, 0.f, 0});
    if (tab.empty()) return true;  // every proportion is 0: the identity
    if (!kf_dropout_masks || !kf_row_seg) {
        set_err("forward: this build of libkaldi_fp16 has no dropout kernels");
        return false;
    }
    const int B = net->B > 0 ? net->B : 1, T = net->T;
    if (B > net->drop_cap) {
        const int cap = (B + 63) / 64 * 64;
        for (int li : net->drop_layers) {
            NetLayer &nl = net->layers[li];
            if (!(nl.drop = (float *)net->dalloc((size_t)cap * nl.L.out_dim * 4))) {
                set_err("forward: alloc dropout masks");
                return false;
            }
        }
        net->drop_cap = cap;
    }
    if (!net->row_seg) {
        net->row_seg = (int32_t *)net->dalloc((size_t)net->max_T * 4);
        net->row_seg_c = (int32_t *)net->dalloc((size_t)net->max_T * 4);
        if (!net->row_seg || !net->row_seg_c) {
            set_err("forward: alloc dropout row maps");
            return false;
        }
    }
    size_t k = 0;
    for (int li : net->drop_layers) {
        NetLayer &nl = net->layers[li];
        if (!(nl.drop_p > 0.f)) continue;
        tab[k++] = KfDropLayer{nl.drop, nl.L.out_dim, nl.L.out_dim, nl.drop_ord, nl.drop_p, 0};
        nl.drop_act = true;
    }
    const int *so = net->B > 1 ? net->seq_off : nullptr;
    if (!ck(kf_dropout_masks((int)tab.size(), tab.data(), B, net->drop_seed, step), "dropout masks") ||
        !ck(kf_row_seg(net->row_seg, so, so ? B : 1, T, 0, 0), "dropout row map") ||
        (net->rs.Tc > 0 && !ck(kf_row_seg(net->row_seg_c, so, so ? B : 1, T, net->rs.Tc0, net->rs.Tc), "dropout row map (compact rows)")))
        return false;
    net->drop_B = B;
    net->drop_live = true;
    return true;
}

// SpecAugment of this forward: which spec-augment layers mask (the switch on and
// a band or a time mask to draw), their storage, and the row_band of each, one launch per
// layer; fwd_layer applies it. The step advances at every forward while the switch is on, masks
// drawn or not. The layer's activation and row_band are made at the first forward that needs
// them: nothing is allocated per step.
bool sa_prepare(KfNet *net) {
    for (int li : net->sa_layers) net->layers[li].sa_act = false;
    if (!sa_active(net)) return true;
    const long long step = net->sa_step;
    net->sa_step = (step + 1) & 0xFFFFFFFFll;
    const int *so = net->B > 1 ? net->seq_off : nullptr;
    for (int li : net->sa_layers) {
        NetLayer &nl = net->layers[li];
        const int dim = nl.L.out_dim, Z = sa_max_bins(nl);
        if (Z <= 0 && !(nl.sa_z > 0)) continue;  // the identity: stays the alias
        if (!kf_specaug_rows || !kf_specaug_apply) {
            set_err("forward: this build of libkaldi_fp16 has no SpecAugment kernels");
            return false;
        }
        // (an MXFP8 consumer through the alias is refused when the switches are set, modes.cpp;
        // nnet_set_row_subsampling admits no spec-augment layer into the compact row set)
        if (!nl.act && !(nl.act = net->dalloc((size_t)net->max_T * dim * 2))) {
            set_err("forward: alloc activation " + nl.L.name);
            return false;
        }
        if (!nl.sa_rows && !(nl.sa_rows = (int32_t *)net->dalloc((size_t)net->max_T * 4))) {
            set_err("forward: alloc SpecAugment rows " + nl.L.name);
            return false;
        }
        // m_n = max(1, floor(m (1 - z) / z)) in double, capped at what an int holds
        int max_kept = 1;
        if (nl.sa_z > 0) {
            const double mn = std::floor((double)nl.sa_m * (1.0 - nl.sa_z) / nl.sa_z);
            max_kept = mn >= 2147483647.0 ? 2147483647 : mn < 1.0 ? 1 : (int)mn;
        }
        if (!ck(kf_specaug_rows(nl.sa_rows, so, so ? net->B : 1, net->T, dim, Z, (float)nl.sa_z, nl.sa_m, max_kept,
                                (unsigned)nl.sa_ord, net->sa_seed, step),
                "spec-augment rows"))
            return false;
        nl.sa_act = true;
    }
    return true;
}

// Training-mode BatchNorm of this forward: every governed layer normalises by its
// own batch statistics while the switch is on. The switches refuse the combinations that do
// not work when they are set (modes.cpp); this is the same rule where the forward would break it.
bool bnt_prepare(KfNet *net) {
    for (int li : net->bnt_layers) net->layers[li].bnt_act = false;
    if (!bnt_active(net)) return true;
    if (!admit(net, Mode::BnTrain, "forward")) return false;
    if (!kf_bn_train_stats || !kf_bn_train_apply) {
        set_err("forward: this build of libkaldi_fp16 has no training-mode BatchNorm kernels");
        return false;
    }
    if ((net->bnt_sites & KF_BN_SITE_CONV) && !kf_bn_block_stats) {
        set_err("forward: this build of libkaldi_fp16 has no block BatchNorm kernels");
        return false;
    }
    for (int li : net->bnt_layers) net->layers[li].bnt_act = net->layers[li].bnt_stat != nullptr;
    return true;
}

int forward_impl(KfNet *net, const void *features, int T) {
    if (!on_device(net, "forward")) return -1;
    if (!refresh_wt(net)) return -1;
    if (T <= 0 || T > net->max_T) {
        set_err("forward: T=" + std::to_string(T) + " outside (0, max_frames]");
        return -1;
    }
    net->T = T;
    net->features = features;
    net->rs = RowSet(T, 0, 0);
    if (net->rsub && net->first_c >= 0 && !net->fp8 && !net->implicit_dz) {
        const int nt = (T - 1) % 3 == 0 ? 0 : net->rs_nt;
        const int tc0 = (T - 1) / 3 + 1;
        if (tc0 >= 4 * nt + 16 && tc0 + nt <= net->maxTc) net->rs = RowSet(T, tc0, nt);
    }
    if (!drop_prepare(net) || !sa_prepare(net) || !bnt_prepare(net) || !sr_prepare(net, "forward")) return -1;
    for (size_t li = 0; li < net->layers.size(); ++li) {
        NetLayer &nl = net->layers[li];
        const void *x = act_of(net, nl.input);
        if (net->rs.Tc && (int)li == net->first_c && !conv_c_on(net)) {  // the conv stack's output on the compact rows
            if (!ck(kf_gather_rows(net->xc, x, (long long)nl.L.in_dim * 2, T, net->rs.Tc0, net->rs.Tc), "row set gather"))
                return -1;
            x = net->xc;
        }
        if (!fwd_layer(net, (int)li, x, T)) return -1;
    }
    return 0;
}

}  // namespace

extern "C" int nnet_forward(KfNet *net, const void *features, int T) {
    kf_take_pending(__func__);
    if (net->ivec_dim) {
        set_err("forward: the network has an ivector input; use nnet_forward_ivector");
        return -1;
    }
    // the sequences nnet_set_sequences gave (their offsets are in seq_off), else one sequence
    net->B = net->seq_row0.empty() ? 0 : (int)net->seq_row0.size() - 1;
    if (net->B > 0 && net->seq_row0.back() != T && drop_active(net)) {
        set_err("forward: T=" + std::to_string(T) + " is not the " + std::to_string(net->seq_row0.back()) +
                " frames of the sequences given to nnet_set_sequences (dropout draws one mask per sequence)");
        return -1;
    }
    if (net->B > 0 && net->seq_row0.back() != T && sa_active(net)) {
        set_err("forward: T=" + std::to_string(T) + " is not the " + std::to_string(net->seq_row0.back()) +
                " frames of the sequences given to nnet_set_sequences (SpecAugment draws one mask per sequence)");
        return -1;
    }
    if (net->B > 0 && net->seq_row0.back() != T) net->B = 0;
    return forward_impl(net, features, T);
}
// forward with per-sequence ivectors: ivectors fp16 [B x ivec_dim] on the device,
// seq_row0 host int[B+1] frame offsets (seq_row0[0] = 0, seq_row0[B] = T)
extern "C" int nnet_forward_ivector(KfNet *net, const void *features, int T, const void *ivectors, int B,
                                    const int *seq_row0) {
    kf_take_pending(__func__);
    if (!on_device(net, "forward_ivector")) return -1;
    // validate everything before touching the device or the network's state
    if (T <= 0 || T > net->max_T) {
        set_err("forward_ivector: T=" + std::to_string(T) + " outside (0, max_frames]");
        return -1;
    }
    if (!net->ivec_dim || !ivectors || B <= 0 || B > T || !seq_row0 || seq_row0[0] != 0 || seq_row0[B] != T) {
        set_err("forward_ivector: needs an ivector input layer, B in [1, T] and seq_row0[0] = 0, seq_row0[B] = T");
        return -1;
    }
    for (int s = 0; s < B; ++s)
        if (seq_row0[s + 1] <= seq_row0[s]) {
            set_err("forward_ivector: empty or unordered sequence " + std::to_string(s));
            return -1;
        }
    if (!net->seq_off) {
        net->seq_off = (int *)net->dalloc(((size_t)net->max_T + 1) * 4);
        if (!net->seq_off) {
            set_err("alloc seq offsets");
            return -1;
        }
    }
    if (bridge_transfer_int32(net->seq_off, seq_row0, (size_t)B + 1)) {
        set_err("upload seq offsets");
        return -1;
    }
    net->ivec = ivectors;
    net->B = B;
    return forward_impl(net, features, T);
}

extern "C" const void *nnet_activation(const KfNet *cnet, const char *layer, int *rows, int *cols) {
    KfNet *net = const_cast<KfNet *>(cnet);
    for (size_t i = 0; i < net->layers.size(); ++i)
        if (net->layers[i].L.name == layer) {
            if (rows) *rows = act_rows(net, (int)i);  // compact rows above the conv stack (row subsampling)
            if (cols) *cols = net->layers[i].L.out_dim;
            return act_of(net, (int)i);
        }
    set_err(std::string("no layer ") + layer);
    return nullptr;
}
