// net_internal.h — the host layer's network state and the helpers its translation units
// share: network.cpp (topology, allocation, parameters), mxfp8.cpp, modes.cpp (the switches and
// which of them combine, data parallel), update.cpp (sgd / update / orthonormal constraint),
// natgrad.cpp, regularize.cpp (dropout, SpecAugment, training-mode BatchNorm), forward.cpp and
// backward.cpp. Nothing here is part of the C-ABI (kf_nnet.h).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "nnet_host.h"

using kf::Layer;
using kf::LayerType;

#define KF_HIDDEN __attribute__((visibility("hidden")))  // internal to libkaldi_fp16_nnet.so

KF_HIDDEN void set_err(const std::string &s);

// The entry points of the newer kernels (update, orthonormal constraint, natural gradient,
// dropout, SpecAugment, training-mode BatchNorm) are weak references: a program that links the
// host layer against a backend without them still links, and the nnet_* call that needs one
// reports it missing.
#pragma weak kf_update_maxchange
#pragma weak kf_update_scratch_bytes
#pragma weak kf_orthonormal_constrain
#pragma weak kf_orthonormal_scratch_bytes
#pragma weak kf_ng_init
#pragma weak kf_ng_default_opts
#pragma weak kf_ng_apply_scratch_bytes
#pragma weak kf_ng_state_scratch_bytes
#pragma weak kf_ng_trx
#pragma weak kf_ng_scales
#pragma weak kf_ng_apply
#pragma weak kf_ng_state
#pragma weak kf_dropout_masks
#pragma weak kf_row_seg
#pragma weak kf_specaug_rows
#pragma weak kf_specaug_apply
#pragma weak kf_bn_train_stats
#pragma weak kf_bn_train_apply
#pragma weak kf_bn_train_bwd_stats
#pragma weak kf_bn_train_bwd_apply
#pragma weak kf_bn_train_bwd_stats_rows
#pragma weak kf_bn_train_bwd_apply_rows
#pragma weak kf_bn_block_stats
#pragma weak kf_bn_block_bwd_stats
#pragma weak kf_bn_train_stats_relu
#pragma weak kf_bn_block_stats_relu
#pragma weak kf_relu_repair_vectors
#pragma weak kf_bn_train_bwd_apply_repair
#pragma weak kf_bn_train_bwd_apply_rows_repair
#pragma weak kf_loss_scale_state_bytes
#pragma weak kf_loss_scale_scratch_bytes
#pragma weak kf_loss_scale_init
#pragma weak kf_loss_scale_set_scale
#pragma weak kf_loss_scale_check
#pragma weak kf_loss_scale_read
#pragma weak kf_update_maxchange_scaled
#pragma weak kf_sgd_flat_scaled
// (a query: against a backend without it nnet_set_row_subsampling decides as it did before it asked)
#pragma weak kf_gemm_wgrad_halo_applies

struct ParamRef {
    std::string name;
    int rows, cols;
    long long off;
};

// an update component (kf_nnet.h nnet_update): one Kaldi nnet3 component's tensors,
// params[first .. first + count), and its options
struct UpdComponent {
    std::string name;
    int first, count;
    float max_change, l2, lr_factor;
    float orthonormal;  // kf_nnet.h nnet_constrain_orthonormal: 0 off, > 0 fixed scale, < 0 floating
};

// an MXFP8 tensor: e4m3 [rows x ld] + E8M0 scales [rows x ld/32] (kf_ops.h)
struct Mx {
    uint8_t *q = nullptr, *s = nullptr;
    int ld = 0;
};

struct NetLayer {
    Layer L;
    int input = -1;  // index into layers, -1 = network input (features)
    int pW = -1, pb = -1, pW2 = -1, pb2 = -1;
    std::vector<int> dt, dh;  // conv: cross product of offsets (Kaldi)
    float *bn_scale = nullptr, *bn_shift = nullptr;    // device, expanded to out width
    float *bn2_scale = nullptr, *bn2_shift = nullptr;  // prefinal small BN
    std::vector<float> hbn[4], hbn2[4];                // host mean,var,gamma,beta
    float bn_eps = 1e-3f, bn_rms = 1.f, bn2_eps = 1e-3f, bn2_rms = 1.f;
    bool has_bn2 = false;
    void *act = nullptr;      // fp16 [maxT x out_dim] (spec-augment: the alias of its input, see act_of)
    bool act_alias = false;
    uint8_t *mask = nullptr;  // relu bits
    void *aux = nullptr;      // tdnnf bottleneck / prefinal big
    void *idct = nullptr;     // fp16 [D x D]
    void *dproj = nullptr;    // attention: fp16 [maxT x affine] gradient of aux (the affine output)
    float *att_scratch = nullptr;  // attention: fp32 [2 x maxT x heads x context]
    float key_scale = 0.f;
    bool per_seq = false;     // runs on the B per-sequence rows (ReplaceIndex(ivector, t, 0) branch)
    int input2 = -100;        // combine-feature-maps: second Append input (-2 = ivector input)
    // small num-filters-in conv (fin not 1 and not a multiple of 32): im2col + GEMM
    int kp = 0;               // padded K (multiple of 64)
    void *im2col = nullptr;   // fp16 [maxT*hout x kp], also reused for dP in backward
    void *wpad = nullptr;     // fp16 [kp x fout], rows >= ntaps*fin zero
    float *gwpad = nullptr;   // fp32 [kp x fout] weight gradient over the padded K
    void *gdb = nullptr;      // fp16 per-sequence gradient [maxT x dim] (combine backward)
    bool bypass = false;
    bool needs_dx = false;
    bool compact = false;     // computed on the supervised row set (nnet_set_row_subsampling)
    // MXFP8 forward (nnet_set_fp8): output / aux copies written by the producing
    // GEMM epilogue, and the weights quantised [N][K] with each splice part padded
    Mx a8, x8, w8, w8b;
    // MXFP8 train step, TDNN-F with a time stride: the affine weight rows for the input
    // gradient, [bottleneck x 2 * pad128(out_dim)] (part p = rows p*bn .. of W2, blocks of 32
    // along out_dim), quantised with the forward copies
    Mx w8d;
    // k-contiguous (transposed) fp16 copy of a short-K forward weight, [N x K], for the
    // fused GEMM's k-contiguous B; refreshed from w16 before a forward after any change
    void *wt = nullptr;
    int wt_pi = -1, wt_K = 0, wt_N = 0;
    // conv input gradient, per-tap transposed weight blocks [fout x fin] (dgrad_wt)
    void *wtd = nullptr;
    // per-sequence dropout (TDNN-F, kf_nnet.h nnet_set_dropout): the current proportion (< 0: no
    // component), the layer's place in the generator's counter, its mask [drop_cap x out_dim]
    // fp32, and whether the current forward drew and applied one
    float drop_p = -1.f;
    int drop_ord = -1;
    float *drop = nullptr;
    bool drop_act = false;
    // training-mode BatchNorm (TDNN-F, kf_nnet.h nnet_set_bn_train): r = the affine's
    // relu output fp16 [max_T x out_dim], the last forward's mean | var | scale | shift (fp32, out_dim
    // each; bn_scale / bn_shift stay the frozen pair), the accumulators count (2 doubles, the
    // second unused) | sum | sumsq in double, all made when the mode is first switched on, and
    // whether the current forward normalised by its own statistics
    // The other sites (nnet_set_bn_train_sites) use the same fields with the BatchNorm's
    // own length (bnt_dim below): a conv layer's r is [max_T x height-out num-filters-out] and its
    // statistics are num-filters-out long; a prefinal layer's r is big-dim wide and the *2 fields
    // are its BatchNorm 1 (r2: the linear output, small-dim wide); a batchnorm-component's r is
    // its input, and bnt_r holds the backward's dz instead (the per-sequence branch only: a
    // frame-level one has no backward and no bnt_r).
    void *bnt_r = nullptr;
    float *bnt_stat = nullptr;
    double *bnt_acc = nullptr;
    bool bnt_act = false;
    void *bnt_r2 = nullptr;
    float *bnt_stat2 = nullptr;
    double *bnt_acc2 = nullptr;
    // ReLU statistics and self-repair (kf_nnet.h nnet_set_self_repair) of the ReLU that
    // BatchNorm 0 above governs: the options (xconfig self-repair-*), the accumulators count (2
    // doubles, the second unused) | deriv_sum [bnt_dim] in double, the last backward's repair vector
    // s [bnt_dim] fp32, both made when the mode first finds the layer a site, and whether the
    // current forward counted (the backward then adds s)
    float sr_scale = 1e-5f;
    double sr_lower = 0.05, sr_upper = 0.95;
    double *sr_acc = nullptr;
    float *sr_s = nullptr;
    bool sr_act = false;
    // spec-augment-layer (kf_nnet.h nnet_set_spec_augment): the layer's ordinal among such layers
    // (-1: another kind), its options, the row_band [max_T] of its last active forward, and
    // whether the current forward masked (act is then the layer's own buffer, not the alias)
    int sa_ord = -1;
    double sa_f = 0.5, sa_z = 0.2;
    int sa_m = 10;
    int32_t *sa_rows = nullptr;
    bool sa_act = false;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The supervised row set of a forward (KfNet::rsub below), the only holder of its numbers:
// compact row c is source row 3c for c < Tc0, then the nt tail rows tail_t0, tail_t0 + 3,
// ... T-1. Every frame position the forward and backward derive from it is named here, once.
// Tc == 0: the forward ran on full rows. With nt == 0 (no tail: (T-1) % 3 == 0, or no row
// set) tail_t0 lies past the last frame, the window is empty and the residues reach frame T-1.
struct RowSet {
    int Tc = 0, Tc0 = 0, nt = 0;  // compact rows, those of frames 3c, tail rows (Tc = Tc0 + nt)
    int tail_t0 = 0;              // first tail frame, T-1-3(nt-1)
    int window_t0 = 0;            // first frame the tail reaches through the conv below: tail_t0 - 2
    int residue_last_frame = 0;   // last input frame of the compact conv's per-residue input gradients
    RowSet() = default;
    RowSet(int T, int Tc0_, int nt_)
        : Tc(Tc0_ + nt_), Tc0(Tc0_), nt(nt_), tail_t0(T - 1 - 3 * (nt_ - 1)), window_t0(tail_t0 - 2),
          residue_last_frame(window_t0 - 1) {}
    // compact row of source row t < T, or -1 when t is not in the set
    int compact_of(int t) const {
        if (t % 3 == 0 && t / 3 < Tc0) return t / 3;
        if (t >= tail_t0 && (t - tail_t0) % 3 == 0 && (t - tail_t0) / 3 < nt) return Tc0 + (t - tail_t0) / 3;
        return -1;
    }
};

struct KfNet {
    std::vector<Layer> all;
    std::vector<NetLayer> layers;
    // Model.ChainOutput (model.go:271-281): the output layer named "output", else the first
    // output layer; backward is seeded there. Trainable layers off its input path (the xent
    // branch) get no gradient (network_backward.go:110-115): their ranges are zeroed.
    int chain_out = -1;
    std::vector<std::pair<long long, long long>> offpath;  // (float offset, count) in grad
    int feat_dim = 0, max_T = 0, T = 0;
    const void *features = nullptr;
    // ivector input: one row per sequence, frames -> sequences by
    // seq_off (device int[B+1]); layers fed from it run on B rows (per_seq)
    int ivec_dim = 0, B = 0;
    const void *ivec = nullptr;
    int *seq_off = nullptr;
    long long nparams = 0;
    std::vector<ParamRef> params;
    float *master = nullptr, *grad = nullptr, *vel = nullptr;
    void *w16 = nullptr;
    // input-gradient ring (three deep: a step's output gradient is not rewritten until the
    // weight gradients of the step after next have read it)
    void *dz[3] = {nullptr, nullptr, nullptr}, *g[3] = {nullptr, nullptr, nullptr};
    void *dbott = nullptr, *edge = nullptr;
    // Weight gradients run on their own stream (nnet_set_wgrad_stream, default on): a layer's
    // dW GEMMs hang off the input-gradient chain (dz -> dbott -> dz below) and overlap it.
    // dbott cycles through three buffers by backward step, so the next layers' affine input
    // gradients never wait for this layer's linear weight gradient.
    void *dbott2 = nullptr, *dbott3 = nullptr;
    void *wg_stream = nullptr, *ev_go = nullptr, *ev_side = nullptr;
    void *ev_step[3] = {nullptr, nullptr, nullptr};  // end of a backward step's side work (ring)
    void *ev_aux = nullptr;  // side-stream launches main joins on the spot (conv tail rows / window)
    void *hp_stream = nullptr;  // high-priority stream for the input-gradient chain
    int wg_side = 1;
    // Implicit dz (nnet_set_implicit_dz, default off, fp16 step): the input-gradient epilogue
    // that produces a TDNN-F layer's g stores no dz = rne(g * bnscale * mask); the layer's
    // affine weight and input gradients read g through the forward's ReLU mask (masked
    // operands, kf_ops.h) with the BN scale folded into W2 (w2s scratch) or the weight
    // gradient's reduction. One full-width fp16 tensor fewer written per TDNN-F layer, but
    // step-neutral on the MI355X (the linear input gradient's saving is spent
    // by the masked affine input gradient on the same chain), so off by default.
    int implicit_dz = 0;
    int main_aff = 0;              // nnet_debug_backward (tests)
    // Row-subsampled train step (nnet_set_row_subsampling, r6). The chain objective reads the
    // output on rows 0 (mod 3) only, and every layer from first_c up (TDNN-F with time
    // stride 0 / 3, linear, prefinal, output) maps row t from rows t, t +- 3 of the layer
    // below; with the splices' clamp at T - 1 the rows those outputs depend on are the rows
    // 0 (mod 3) plus a tail of rows T-1, T-4, ... as deep as the layers. Those layers run on
    // that compact set: compact row c is source row 3c for c < Tc0, else
    // (T-1) - 3 (Tc-1-c); a splice of +-3 source rows is +-1 compact row. At the boundary
    // (c = Tc0 - 1 whose +3 row is T-1 = compact Tc-1, and tail row Tc0 whose -3 row is not
    // in the set) the tail row Tc0 is a scratch slot: after each linear GEMM it receives a
    // copy of the bottleneck's row Tc - 1, so row Tc0 - 1's +1 neighbour reads row T-1, and
    // its bottleneck gradient is zeroed after the affine input gradient (its true gradient,
    // as every row outside the set, is zero). Its own values and those its wrong neighbour
    // reaches stay more than the tail's depth away from every row with a gradient.
    int rsub = 0;                  // 3: on
    int first_c = -1;              // lowest compact layer (its input: a conv, full rows)
    // the conv below first_c evaluated on the compact rows only (its output frames 3c and the
    // tail; time-strided halo operand, kf_ops.h KfOperand.tmul): its activation and mask are
    // then in compact rows and first_c reads them directly. Its backward stays on full rows
    // (the input gradient scattered back). KF_RSUB_CONV=0 at nnet_set_row_subsampling: off; off
    // too where the halo weight-gradient kernel does not cover the conv's time-strided rows
    // (kf_ops.h kf_gemm_wgrad_halo_applies).
    int conv_c = 0;
    int rs_nt = 0;                 // tail rows when (T - 1) % 3 != 0
    RowSet rs;                     // the row set of the current forward (rs.Tc == 0: full rows)
    int maxTc = 0;
    void *xc = nullptr;            // first_c's input, gathered to compact rows
    void *dzc = nullptr;           // first_c's input gradient in compact rows
    uint8_t *mc = nullptr;         // the mask of first_c's input, compact rows
    // bottleneck-gradient row mask [maxTc x rm_bn bits]: all ones but the scratch row Tc0
    // (the TDNN-F affine input gradient zeroes that row in its epilogue)
    uint8_t *rowmask = nullptr;
    int rm_bn = 0, rm_tc0 = -1, rm_tc = -1;
    long long stall_side = 0;      // nnet_debug_backward (tests): spin before side work
    bool dz_imp[3] = {false, false, false};  // dz[i] was left implicit by the producing epilogue
    bool dz_edge[3] = {false, false, false}; // row T of dz[i] already holds the strided TDNN-F edge sum
    void *w2s = nullptr;              // [kaff x dout] fp16: W2 with the BN scale folded in
    // nnet_backward_xent: the xent branch's gradient at the branch point, fp16 [max_T x dim],
    // made at the first call (backward.cpp branch_pass)
    void *gx = nullptr;
    void *dbott_last = nullptr;  // the dbott buffer of the last TDNN-F / prefinal step (tests)
    void *dz_last = nullptr;     // the input gradient the last backward step handed down (tests)
    size_t edge_half = 0;
    int fp8 = 0;
    int fp8_dgrad = 1;  // nnet_set_fp8(net, 2): MXFP8 forward, fp16 affine input gradients (tests)
    // MXFP8 copies of dz[0] / dz[1] written by the producing input-gradient epilogue
    // (out8_src = 1) for a TDNN-F layer's affine input gradient, and the layer each holds
    Mx dz8[3];
    int dz8_layer[3] = {-1, -1, -1};
    bool wt_dirty = true;  // the transposed weight copies need a refresh (NetLayer::wt)
    // nnet_update: the components, and their device tables (kf_ops.h KfUpdSegment / KfUpdComp),
    // scratch and stats, made at the first update and again after an option changed
    std::vector<UpdComponent> comps;
    bool upd_dirty = true;
    int upd_nseg = 0;
    void *upd_segs = nullptr, *upd_comps = nullptr, *upd_scratch = nullptr;
    float *upd_stats = nullptr;
    bool upd_ran = false;  // upd_stats holds an update's report
    // dynamic loss scale (kf_nnet.h nnet_set_loss_scale): the switch, the device state
    // (kf_ops.h kf_loss_scale_*; made at the first set call, kept when the mode goes off) and the
    // check pass's per-workgroup flags
    bool ls_on = false;
    void *ls_state = nullptr, *ls_flags = nullptr;
    // nnet_constrain_orthonormal: the constrained components (indices into comps, in comps'
    // order), their matrix table on the host and on the device (kf_ops.h KfOrthoMat), scratch
    // and stats, made at the first call and again after nnet_set_component_orthonormal
    bool ort_dirty = true;
    std::vector<int> ort_comps;
    std::vector<KfOrthoMat> ort_mats;
    void *ort_mats_dev = nullptr, *ort_scratch = nullptr;
    float *ort_stats = nullptr;
    size_t ort_cap = 0;         // entries ort_mats_dev / ort_stats hold
    long long ort_scratch_bytes = 0;
    bool ort_ran = false;  // ort_stats holds a call's report
    // natural-gradient preconditioning (kf_nnet.h nnet_set_natural_gradient): the preconditioner
    // and component tables on the host and on the device (kf_ops.h KfNgPre / KfNgComp), state,
    // statistics, scratch and report, all made when the switch is set
    bool ng_on = false;
    KfNgOpts ng_opts{};
    std::vector<KfNgPre> ng_pres;
    std::vector<KfNgComp> ng_comps;
    std::vector<int> ng_pre_comp, ng_pre_side;  // per preconditioner: update component, 0 in / 1 out
    std::vector<int> ng_of_param;               // weight tensor -> its entry of ng_comps, or -1
    std::vector<char> ng_issued;                // per entry: this backward issued its statistics
    void *ng_pres_dev = nullptr, *ng_comps_dev = nullptr, *ng_w16 = nullptr, *ng_h = nullptr;
    void *ng_apply_scratch = nullptr, *ng_state_scratch = nullptr;
    float *ng_w32 = nullptr, *ng_stat = nullptr, *ng_report = nullptr;
    double *ng_sc = nullptr;
    long long ng_t = 0;      // steps so far: t < 10 or t % update_period == 0 updates the state
    bool ng_updating = false;  // this backward's steps
    bool ng_ran = false;     // ng_report holds a backward's report
    // per-sequence dropout (kf_nnet.h nnet_set_dropout): the layers with a component,
    // the switch, the generator's key and step, the sequence boundaries nnet_set_sequences gave
    // (host copy; seq_off holds them on the device), the row -> sequence maps of the current
    // forward (full rows / compact rows) and the sequences the mask tables hold
    std::vector<int> drop_layers;
    int drop_on = 0;
    unsigned long long drop_seed = 0;
    long long drop_step = 0;
    std::vector<int> seq_row0;
    int32_t *row_seg = nullptr, *row_seg_c = nullptr;
    int drop_cap = 0, drop_B = 0;
    bool drop_live = false;  // the current forward applied masks
    // SpecAugment (kf_nnet.h nnet_set_spec_augment): the spec-augment layers, the
    // switch, the generator's key and the feature's own step
    std::vector<int> sa_layers;
    int sa_on = 0;
    unsigned long long sa_seed = 0;
    long long sa_step = 0;
    // training-mode BatchNorm (kf_nnet.h nnet_set_bn_train): the layers the switch
    // governs (the tdnnf-layers), the switch, and the backward's a | b columns (fp32, the widest
    // governed layer's out_dim each; one pair: the chain stream runs the layers in order)
    // bnt_sites: the kinds of layer the switch governs (KF_BN_SITE_*); bnt_layers follows it.
    std::vector<int> bnt_layers;
    int bnt_sites = 1;  // KF_BN_SITE_TDNNF
    int bnt_on = 0;
    float *bnt_ab = nullptr;
    int bnt_w = 0;
    // nnet_set_bn_train_rows: KF_BN_ROWS_SUBSAMPLED lets the switch and row subsampling
    // be on together; a governed BatchNorm of a compact layer then takes its statistics from the
    // rows c < Tc0 of a compact forward (bnt_stat_rows below)
    int bnt_rows = 0;  // KF_BN_ROWS_ALL
    // ReLU statistics and self-repair (kf_nnet.h nnet_set_self_repair): the switch, and
    // the table of the current forward's sites (kf_ops.h KfRepairSite) on the host and on the device,
    // made again when the sites or an option changed (regularize.cpp sr_prepare)
    int sr_on = 0;
    std::vector<int> sr_sites;
    std::vector<KfRepairSite> sr_tab;
    void *sr_tab_dev = nullptr;
    size_t sr_tab_cap = 0;
    bool sr_dirty = true;
    // data parallel (kf_dp.h): gradient buckets exchanged during the backward
    KfDp *dp = nullptr;
    std::vector<int> dp_after;  // bucket j is issued after backward step dp_after[j]
    std::vector<long long> dp_begin, dp_end;
    bool dp_early = false;  // nnet_dp_debug_early: every bucket issued before the backward (tests)
    std::vector<void *> allocs;

    void *dalloc(size_t bytes) {
        void *p = bridge_gpu_malloc(bytes ? bytes : 16);
        if (p) allocs.push_back(p);
        return p;
    }
    // gives a dalloc'ed block back before the net is closed (NULL: nothing)
    void dfree(void *p) {
        const auto it = std::find(allocs.begin(), allocs.end(), p);
        if (!p || it == allocs.end()) return;
        allocs.erase(it);
        bridge_gpu_free(p);
    }
    ~KfNet() {
        if (wg_stream) bridge_gpu_sync();
        kf_event_free(ev_go);
        kf_event_free(ev_side);
        for (void *e : ev_step) kf_event_free(e);
        kf_event_free(ev_aux);
        kf_stream_free(wg_stream);
        kf_stream_free(hp_stream);
        for (void *p : allocs) bridge_gpu_free(p);
    }
};

// the helpers below are internal to libkaldi_fp16_nnet.so: not exported
#pragma GCC visibility push(hidden)

inline KfAttention att_args(const NetLayer &nl, int T) {
    const Layer &L = nl.L;
    const int context = 1 + L.num_left + L.num_right;
    return KfAttention{nl.aux, (long long)L.num_heads * (2 * L.key_dim + L.value_dim + context), T, L.num_heads,
                       L.key_dim, L.value_dim, context, L.num_left, L.att_stride, nl.key_scale};
}

inline KfOperand op_base(const void *p, long long ld, int rows, int cols, int kcontig) {
    KfOperand d;
    memset(&d, 0, sizeof d);
    d.base = p;
    d.ld = ld;
    d.nrows = rows;
    d.ncols = cols;
    d.kcontig = kcontig;
    d.nparts = 1;
    d.part_width = cols;
    d.T = rows;
    d.hout = 1;
    d.hsrc = 1;
    d.hmul = 0;
    d.hdiv = 1;
    d.tpolicy = KF_ZERO;
    for (int i = 0; i < KF_MAX_PARTS; ++i) d.edge_t[i] = -1;
    return d;
}
// [x(t+dt0) | x(t+dt1)] over T rows of width d (forward.go:699-790)
inline KfOperand op_splice(const void *p, int T, int d, int dt0, int dt1, int policy, int kcontig) {
    KfOperand o = op_base(p, d, T, 2 * d, kcontig);
    o.nparts = 2;
    o.part_width = d;
    o.dt[0] = dt0;
    o.dt[1] = dt1;
    o.tpolicy = policy;
    return o;
}
// im2col of a conv layer input [T x hin*fin] -> rows (t,h) < T*hout, cols (o,f)
inline KfOperand op_im2col(const NetLayer &nl, const void *x, int T, int kcontig) {
    const Layer &L = nl.L;
    const int noff = (int)nl.dt.size();
    KfOperand o = op_base(x, (long long)L.hin * L.fin, T * L.hout, noff * L.fin, kcontig);
    o.nparts = noff;
    o.part_width = L.fin;
    o.T = T;
    o.hout = L.hout;
    o.hsrc = L.hin;
    o.hmul = L.hsub;
    o.hdiv = 1;
    o.tpolicy = KF_ZERO;
    for (int i = 0; i < noff; ++i) {
        o.dt[i] = nl.dt[i];
        o.dh[i] = nl.dh[i];
    }
    return o;
}
// transpose-conv gather of dz [(t,h) x fout]: rows (t',h') < T*hin, cols (o,n)
inline KfOperand op_col2im(const NetLayer &nl, const void *dz, int T) {
    const Layer &L = nl.L;
    const int noff = (int)nl.dt.size();
    KfOperand o = op_base(dz, (long long)L.hout * L.fout, T * L.hin, noff * L.fout, 1);
    o.nparts = noff;
    o.part_width = L.fout;
    o.T = T;
    o.hout = L.hin;
    o.hsrc = L.hout;
    o.hmul = 1;
    o.hdiv = L.hsub;
    o.tpolicy = KF_ZERO;
    for (int i = 0; i < noff; ++i) {
        o.dt[i] = -nl.dt[i];
        o.dh[i] = -nl.dh[i];
    }
    return o;
}
// weights W[nparts*rows x width] read as B'[j][(p, n)] = W[p*rows + j][n]
inline KfOperand op_wrows(const void *W, int nparts, int rows, int width) {
    KfOperand o = op_base(W, width, rows, nparts * width, 1);
    o.nparts = nparts;
    o.part_width = width;
    o.T = nparts * rows;
    for (int p = 0; p < nparts; ++p) o.dt[p] = p * rows;
    return o;
}
inline KfEpilogue epi0() {
    KfEpilogue e;
    memset(&e, 0, sizeof e);
    e.alpha = 1.f;
    return e;
}

inline void *wptr(KfNet *net, int pi) {
    return pi < 0 ? nullptr : (char *)net->w16 + net->params[pi].off * 2;
}
inline float *gptr(KfNet *net, int pi) { return pi < 0 ? nullptr : net->grad + net->params[pi].off; }
bool ck(int rc, const char *what);
// a network from nnet_create_layout has no device storage
bool on_device(const KfNet *net, const char *what);
// the layer of that name, or NULL (also for a null net or name)
NetLayer *find_layer(KfNet *net, const char *name);
// a list getter's answer: the first n entries to idx (may be NULL), the list's length returned
inline int list_get(const std::vector<int> &v, int *idx, int n) {
    for (int i = 0; idx && i < n && i < (int)v.size(); ++i) idx[i] = v[i];
    return (int)v.size();
}

// ---- the modes that cannot all be combined (modes.cpp: the table) ----
enum class Mode { Fp8, ImplicitDz, RowSubsampling, NaturalGradient, DataParallel, Dropout, BnTrain, SpecAugment,
                  LossScale, SelfRepair,
                  BackwardN /* nnet_backward_n: never "on", only refused */,
                  XentBackward /* nnet_backward_xent: never "on", only refused */ };
// may `turning_on` be switched on (or nnet_backward_n / nnet_backward_xent run) beside the modes that are on? false
// with the error text set, "<fn>: not supported <the mode that is on>[: <reason>]"
bool admit(KfNet *net, Mode turning_on, const char *fn);

inline bool is_trainable(LayerType t) {
    return t == LayerType::ConvReluBN || t == LayerType::TDNNF || t == LayerType::Linear ||
           t == LayerType::Prefinal || t == LayerType::Output || t == LayerType::Attention;
}

// affine width of an attention layer: heads x (key + value + query key + query context)
inline int att_affine(const Layer &L) {
    const int ctx = 1 + L.num_left + L.num_right;
    return L.num_heads * (2 * L.key_dim + L.value_dim + ctx);
}

// dropout is switched on and the network has a layer it applies to (nnet_set_dropout)
inline bool drop_active(const KfNet *net) { return net->drop_on && !net->drop_layers.empty(); }
// SpecAugment is switched on and the network has a spec-augment layer (nnet_set_spec_augment)
inline bool sa_active(const KfNet *net) { return net->sa_on && !net->sa_layers.empty(); }
// training-mode BatchNorm is switched on and the network has a layer it governs (nnet_set_bn_train)
inline bool bnt_active(const KfNet *net) { return net->bnt_on && !net->bnt_layers.empty(); }
// a self-repair site (kf_nnet.h nnet_set_self_repair): a governed layer with a ReLU below its BatchNorm 0
inline bool sr_site_type(LayerType t) {
    return t == LayerType::TDNNF || t == LayerType::Prefinal || t == LayerType::ConvReluBN;
}
// self-repair is switched on and the training-mode BatchNorm sites hold a layer with a ReLU: what
// the table of mode conflicts calls on (modes.cpp)
inline bool sr_switched(const KfNet *net) {
    if (!net->sr_on) return false;
    for (int li : net->bnt_layers)
        if (sr_site_type(net->layers[li].L.type)) return true;
    return false;
}
// ... and training-mode BatchNorm is on: the passes count and repair
inline bool sr_active(const KfNet *net) { return sr_switched(net) && bnt_active(net); }
// the current forward's sites get their accumulators, repair vectors and table (regularize.cpp);
// sets every layer's sr_act
bool sr_prepare(KfNet *net, const char *fn);
// the length of a layer's BatchNorm statistics (kf_nnet.h nnet_bn_dim): which = 1 is a prefinal
// layer's second BatchNorm
inline int bnt_dim(const NetLayer &nl, int which) {
    const Layer &L = nl.L;
    if (L.type == LayerType::ConvReluBN) return L.fout;
    if (L.type == LayerType::Prefinal) return which ? L.small_dim : L.big_dim;
    return L.out_dim;
}
// Z = min(D, floor(D f + 0.5)): the widest band of a spec-augment layer
inline int sa_max_bins(const NetLayer &nl) {
    return std::min(nl.L.out_dim, (int)((double)nl.L.out_dim * nl.sa_f + 0.5));
}

// the row -> sequence map (KfEpilogue.row_seg) of a GEMM whose rows are a compact layer's
// (the compact row set when the forward has one) or the forward's frames
inline const int32_t *drop_rows(const KfNet *net, bool compact) {
    return compact && net->rs.Tc > 0 ? net->row_seg_c : net->row_seg;
}

// rows a layer's activations / gradients hold in the current forward
inline int rows_of(const KfNet *net, int idx) {
    return (idx >= 0 && net->rs.Tc > 0 && net->layers[idx].compact) ? net->rs.Tc : net->T;
}
// The conv below the compact layers under training-mode BatchNorm (KF_BN_SITE_CONV):
// its statistics run over all rows like every other conv's, so it runs on full rows and the first
// compact layer reads it gathered (the path KF_RSUB_CONV=0 selects). bnt_act is the current
// forward's, set before its first layer runs.
inline bool conv_c_on(const KfNet *net) {
    return net->conv_c && net->first_c >= 0 && !net->layers[net->layers[net->first_c].input].bnt_act;
}
// the conv below the compact layers, evaluated on the compact rows (KfNet.conv_c)
inline bool conv_compact(const KfNet *net, int idx) {
    return net->rs.Tc > 0 && conv_c_on(net) && idx >= 0 && idx == net->layers[net->first_c].input;
}
// the rows the training-mode statistics of layer idx run over in the current forward:
// the rows c < Tc0 (source rows 3c) of a compact layer in a compact forward, else every row
inline int bnt_stat_rows(const KfNet *net, int idx) {
    return (idx >= 0 && net->rs.Tc > 0 && net->layers[idx].compact) ? net->rs.Tc0 : rows_of(net, idx);
}
// rows a layer's activation holds in the current forward
inline int act_rows(const KfNet *net, int idx) {
    return conv_compact(net, idx) ? net->rs.Tc : rows_of(net, idx);
}
inline const void *act_of(KfNet *net, int idx) {
    if (idx == -2) return net->ivec;
    if (idx < 0) return net->features;
    NetLayer &nl = net->layers[idx];
    // (a spec-augment layer is an alias of its input unless this forward masked it)
    return nl.act_alias && !nl.sa_act ? act_of(net, nl.input) : nl.act;
}

// ---- MXFP8 forward (mxfp8.cpp: set-up and weight quantisation) ----
// the MXFP8 weight copies from the fp16 weights (alloc: the first time)
bool quantise_weights(KfNet *net, bool alloc);
// "layer <name> would read the unmasked MXFP8 copy of a spec-augment layer's input", or ""
std::string sa_mx_conflict(const KfNet *net);
inline int pad128(int x) { return (x + 127) / 128 * 128; }
// MXFP8 operand over an Mx tensor of T rows: plain, or spliced [x(t+dt0) | x(t+dt1)]
inline KfOperand op_mx(const Mx &m, int T, int nparts, int dt0, int dt1) {
    KfOperand o = op_base(m.q, m.ld, T, nparts * m.ld, 1);
    if (nparts == 2) {
        o.nparts = 2;
        o.part_width = m.ld;
        o.dt[0] = dt0;
        o.dt[1] = dt1;
        o.tpolicy = KF_CLAMP;
    }
    o.fmt = KF_FMT_MXFP8;
    o.scales = m.s;
    o.lds = m.ld / 32;
    return o;
}
inline KfOperand op_mxw(const Mx &m, int N) {
    KfOperand o = op_base(m.q, m.ld, N, m.ld, 1);
    o.fmt = KF_FMT_MXFP8;
    o.scales = m.s;
    o.lds = m.ld / 32;
    return o;
}
inline void set_out8(KfEpilogue &E, const Mx &m) {
    if (!m.q) return;
    E.out8 = m.q;
    E.ldo8 = m.ld;
    E.scale8 = m.s;
}
// MXFP8 copy of a layer's input, or NULL (fp8 off / producer without one)
inline const Mx *in8(KfNet *net, const NetLayer &nl) {
    if (!net->fp8 || nl.input < 0) return nullptr;
    const NetLayer &p = net->layers[nl.input];
    if (p.act_alias) return in8(net, p);
    return p.a8.q ? &p.a8 : nullptr;
}

// ---- launches beside the current stream (forward conv tail, backward conv window) ----
// The caller has made the weight-gradient stream current behind its own work. Runs the
// launch there, marks its end with ev_aux and makes `back` current again; the caller joins
// later with aux_join. `what` prefixes the error texts ("forward: conv tail").
template <class F>
inline bool side_launch(KfNet *net, void *back, const char *what, F &&launch) {
    const bool ok = launch();
    const bool rec = kf_event_record(net->ev_aux, net->wg_stream) == 0;
    kf_set_stream(back);
    if (ok && !rec) set_err(std::string(what) + " event");
    return ok && rec;
}
inline bool aux_join(KfNet *net, void *st, const char *what) {
    if (kf_stream_wait(st, net->ev_aux) == 0) return true;
    set_err(std::string(what) + " join");
    return false;
}

#pragma GCC visibility pop
