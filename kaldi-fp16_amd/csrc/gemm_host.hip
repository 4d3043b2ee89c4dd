// gemm_host.hip — what the GEMM and conv dispatch units share on the host (gemm_host.h): the
// kf_last_error() slot, operand validation and conversion, the profiler records' algorithmic
// byte counts and the kf_gemm_trace launch counter.
#include "gemm_host.h"

KF_DECLARE_ERR(kf)

extern "C" const char *kf_last_error(void) { return kf_err_.get(); }
extern "C" void kf_clear_error(void) { kf_err_.clear(); }
void kf_report_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    kf_err_.set(fmt, ap);
    va_end(ap);
}

// algorithmic HBM bytes (kf_gemm_alg_bytes, gemm_host.h)
double op_src_bytes(const OpD &o, int f8) {
    // geometry is in 2-byte units, also for MXFP8 (there: payload bytes)
    double b = o.simple ? (double)o.nrows * o.ncols * 2.0 : (double)o.T * (o.hsrc > 0 ? o.hsrc : 1) * o.pw * 2.0;
    if (f8) b += b / 32.0;  // one E8M0 scale per 32 e4m3 values
    if (o.mk) b += b / 16.0;  // one mask bit per fp16 element
    return b;
}
double epi_bytes(const KfEpilogue &E, long long M, long long N) {
    const double mn = (double)M * N;
    double b = 0;
    if (E.out) b += mn * 2 * (E.beta != 0.f ? 2 : 1);
    if (E.out2) b += mn * 2;
    if (E.resid) b += mn * 2;
    if (E.mask_out) b += mn / 8;
    if (E.mask_in) b += mn / 8;
    if (E.out8) b += mn + mn / 32;
    return b;
}
double kf_gemm_alg_bytes(const OpD &a, const OpD &b, const KfEpilogue &E, long long M, long long N) {
    return op_src_bytes(a, 0) + op_src_bytes(b, 0) + epi_bytes(E, M, N);
}

bool to_dev(const KfOperand &d, OpD &o, const char *name) {
    if (!d.base) {
        kf_report_error("operand %s: null base", name);
        return false;
    }
    if (d.nparts < 1 || d.nparts > KF_MAX_PARTS || d.part_width <= 0 || d.hout < 1 || d.hdiv < 1 ||
        (d.hdiv & (d.hdiv - 1)) || d.hdiv > 8) {
        kf_report_error("operand %s: bad addressing (nparts=%d width=%d hout=%d hdiv=%d)", name,
                        d.nparts, d.part_width, d.hout, d.hdiv);
        return false;
    }
    if (d.part_width % 8 != 0 || d.ncols % 8 != 0 || d.ld % 8 != 0 || ((uintptr_t)d.base & 15)) {
        kf_report_error("operand %s: columns / ld / base must be 16-byte granular", name);
        return false;
    }
    if (d.hout > 1 && (long long)(d.hout + BK) * d.hout >= 65536) {
        kf_report_error("operand %s: hout %d too large", name, d.hout);
        return false;
    }
    const bool f8 = d.fmt == KF_FMT_MXFP8;
    if (d.fmt != KF_FMT_FP16 && !f8) {
        kf_report_error("operand %s: unknown format %d", name, d.fmt);
        return false;
    }
    if (f8 && (!d.kcontig || d.hout != 1 || d.ncols % 128 || d.part_width % 128 || d.ld % 16 ||
               !d.scales || d.lds <= 0 || d.nparts > 2)) {
        kf_report_error("operand %s: MXFP8 needs a k-contiguous operand with hout 1, <= 2 parts, "
                        "ncols / part_width multiples of 128, ld multiple of 16 and scales", name);
        return false;
    }
    memset(&o, 0, sizeof o);
    o.base = (const h16 *)d.base;
    // MXFP8: 2-byte units for the byte movers (ld, ncols, part width halved)
    const int u = f8 ? 2 : 1;
    o.ld = d.ld / u;
    o.nrows = d.nrows;
    o.ncols = d.ncols / u;
    o.nparts = d.nparts;
    o.pw = d.part_width / u;
    o.sc = f8 ? d.scales : nullptr;
    o.lds = f8 ? (unsigned)d.lds : 0;
    o.pw8 = f8 ? d.part_width : 0;
    o.T = d.T;
    o.hout = d.hout;
    o.hsrc = d.hsrc;
    o.hmul = d.hmul;
    o.hshift = d.hdiv == 1 ? 0 : d.hdiv == 2 ? 1 : d.hdiv == 4 ? 2 : 3;
    o.tclamp = d.tpolicy == KF_CLAMP;
    o.p64 = o.pw % BK == 0;
    o.inv_hout = (65536u + d.hout - 1) / d.hout;
    bool edges = false;
    for (int i = 0; i < KF_MAX_PARTS; ++i) {
        o.dt[i] = d.dt[i];
        o.dh[i] = d.dh[i];
        o.et[i] = i < d.nparts ? d.edge_t[i] : -1;
        o.er[i] = d.edge_row[i];
        if (i < d.nparts && d.edge_t[i] >= 0) edges = true;
    }
    o.simple = d.nparts == 1 && d.hout == 1 && d.dt[0] == 0 && !edges;
    o.edges = edges;
    if (d.mask) {
        if (f8 || d.hout != 1 || d.mask_rows < 0) {
            kf_report_error("operand %s: a mask needs an fp16 operand with hout 1", name);
            return false;
        }
        o.mk = d.mask;
        const long long lim = (long long)d.mask_rows * d.ld * 2;
        o.mlim = lim > 0xFFFFFFF0LL ? 0xFFFFFFF0u : (unsigned)lim;
    }
    if (d.tmul < 0 || d.t0 < 0 || (d.tmul > 1 && (f8 || d.hout < 2))) {
        kf_report_error("operand %s: time-strided rows (tmul=%d t0=%d) need an fp16 conv operand", name, d.tmul, d.t0);
        return false;
    }
    o.tmul = d.tmul > 1 ? d.tmul : 1;
    o.t0 = d.t0;
    o.ldb = (unsigned)(d.ld * 2 / u);
    o.pwb = (unsigned)(d.part_width * 2 / u);
    // 32-bit byte offsets (buffer addressing): the largest source row must fit
    long long rows = d.nrows;
    if (!o.simple) {
        rows = d.T + 2;
        for (int i = 0; i < d.nparts; ++i)
            if (d.edge_t[i] >= 0 && d.edge_row[i] + 1 > rows) rows = d.edge_row[i] + 1;
    }
    if (rows * d.ld * 2 / u >= (1LL << 32) - 64 || (f8 && rows * d.lds >= (1LL << 32) - 64)) {
        kf_report_error("operand %s: %lld x %lld elements exceed 32-bit buffer addressing", name, rows,
                        d.ld);
        return false;
    }
    return true;
}

// diagnostics: stamp the gemm_kernel launch number `at` (fused and wgrad launches, counted
// from this call): phase stamps of block `blk` and {start, end, hw id} of every block
// (wall_clock64 ticks, 100 MHz). buf holds 64 + 3 * blocks words; null = off
static unsigned long long *g_gemm_trace = nullptr;
static int g_gemm_trace_at = -1, g_gemm_trace_blk = 0, g_gemm_launches = 0;
extern "C" void kf_gemm_trace(unsigned long long *buf, int at, int blk) {
    g_gemm_trace = buf;
    g_gemm_trace_at = at;
    g_gemm_trace_blk = blk;
    g_gemm_launches = 0;
}
unsigned long long *kf_gemm_trace_take(int *blk) {
    if (!g_gemm_trace || g_gemm_launches++ != g_gemm_trace_at) return nullptr;
    *blk = g_gemm_trace_blk;
    return g_gemm_trace;
}
