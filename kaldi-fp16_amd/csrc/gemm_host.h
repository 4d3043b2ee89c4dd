// gemm_host.h — host layer shared by the GEMM and conv dispatch units (gemm_fused*.hip,
// gemm_wgrad.hip, conv_halo.hip, conv_wgrad.hip, gemm_abi.hip): operand validation and
// conversion (KfOperand -> OpD), operand kinds, the algorithmic byte counts of the profiler
// records, the conv tap geometry, and the entry points one dispatch unit offers another.
// gemm_host.hip owns the kf_last_error() slot; every unit writes it with kf_report_error.
#pragma once
#include <algorithm>

#include "gemm_common.h"

// ---- defined in gemm_host.hip
// Algorithmic HBM bytes of one GEMM launch: each operand's SOURCE tensor read once
// (an implicit splice / im2col operand reads its [T x hsrc x part] source, not the
// K-expanded view), the epilogue's tensors read / written once, the fp32 weight
// gradient written once. The floor a perfect-reuse kernel would move.
double kf_gemm_alg_bytes(const OpD &a, const OpD &b, const KfEpilogue &E, long long M, long long N);

// ---- conv halo dispatch (conv_halo.hip, conv_wgrad.hip): 1 launched, 0 not applicable (the
// caller runs the im2col GEMM), -1 error
int kf_conv_wgrad_halo_try(int M, int N, int K, const OpD &a, const OpD &b, float *dW, long long ldw,
                           float *bias_grad, int accumulate);
// the weight-gradient halo plan covers the product (no launch)
bool kf_conv_wgrad_halo_applies(int M, int N, int K, const OpD &a, const OpD &b);
// kf_halo_debug_last's record (kf_ops.h): what the calling thread's last conv_halo_plan
// (kind 1) / conv_wgrad_halo_plan (kind 2) chose. v[0] = kind, v[1] = taken, then the
// fields in kf_ops.h's order. Host only; never read by a launch.
constexpr int KF_HALO_DBG_N = 16;
int *kf_halo_dbg_begin(int kind);  // zeroes the record, sets v[0] = kind; returns v

// ---- split-K reduce of the weight gradients' fp32 slabs (gemm_wgrad.hip)
void kf_wgrad_reduce(const float *slab, const float *bias_slab, int splits, int M, int N, float *dW,
                     long long ldw, float *bias_grad, int accumulate, const float *cs = nullptr);

#pragma GCC visibility push(hidden)
// validates d and converts it; false with the error text set
bool to_dev(const KfOperand &d, OpD &o, const char *name);
double op_src_bytes(const OpD &o, int f8);
double epi_bytes(const KfEpilogue &E, long long M, long long N);
// kf_gemm_trace: the stamp buffer when this gemm_kernel launch (fused and wgrad launches
// share one counter) is the one to stamp, else null; *blk = the block whose phases to stamp
unsigned long long *kf_gemm_trace_take(int *blk);
// conv_halo_kernel (conv_halo.hip) for a fused product on a conv im2col / col2im operand
int conv_halo_try(int M, int N, int K, const OpD &a, const OpD &b, int bm, bool bkc, const KfEpilogue &E);
// splice_once_kernel (splice_once.hip) for a long-K N = 160 / 320 product on a two-part spliced A
// whose 128x160 tiles fit one round of workgroups: 1 launched, 0 not applicable (the caller runs the tiled
// kernel), -1 error
int splice_once_try(int M, int N, int K, const OpD &a, const OpD &b, bool bkc, const KfEpilogue &E);
#pragma GCC visibility pop

static inline int op_mode(const OpD &o) {
    if (o.simple) return OP_SIMPLE;
    if (o.nparts <= 2 && o.hout == 1 && o.hmul == 0 && o.hshift == 0) return OP_P2;
    return OP_GEN;
}
// the reduction-major general stager has no edge-row path
static inline bool mn_gen_ok(const OpD &o, const char *name) {
    if (op_mode(o) == OP_GEN && o.edges) {
        kf_report_error("operand %s: edge rows need a time-only (<= 2 part) reduction-major operand", name);
        return false;
    }
    return true;
}

static inline KfOperand plain_operand(const void *p, long long ld, int rows, int cols, int kcontig) {
    KfOperand d;
    memset(&d, 0, sizeof(d));
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

// ---------------------------------------------------------------------------
// Tap geometry of a conv im2col operand `a` for the halo kernels (conv_halo.hip's header
// comment): the taps' time extent, the height padding and the halo image's rows per parity.
// ---------------------------------------------------------------------------
struct TapGeom {
    int dtmin, dtmax;
    int pad;  // zero heights below the source (max(0, -min dh))
    int hpe;  // image rows per height parity: ceil(padded heights / hmul), the least pitch
};
static inline TapGeom tap_geometry(const OpD &a) {
    int dtmin = 1 << 20, dtmax = -(1 << 20), dhmin = 1 << 20, dhmax = -(1 << 20);
    for (int p = 0; p < a.nparts; ++p) {
        dtmin = std::min(dtmin, a.dt[p]);
        dtmax = std::max(dtmax, a.dt[p]);
        dhmin = std::min(dhmin, a.dh[p]);
        dhmax = std::max(dhmax, a.dh[p]);
    }
    TapGeom g{dtmin, dtmax, std::max(0, -dhmin), 0};
    const int maxshp = (a.hout - 1) * a.hmul + dhmax + g.pad;
    const int HP = std::max(a.hsrc + g.pad, maxshp + 1);
    g.hpe = (HP + a.hmul - 1) / a.hmul;
    return g;
}
// ctap[p]: halo row offset of tap p in an image of hpe (>= g.hpe) rows per parity
static inline void tap_rows(const OpD &a, const TapGeom &g, int hpe, int *ctap) {
    for (int p = 0; p < a.nparts; ++p) {
        const int x = a.dh[p] + g.pad;
        ctap[p] = (a.dt[p] - g.dtmin) * hpe * a.hmul + (x % a.hmul) * hpe + x / a.hmul;
    }
}
