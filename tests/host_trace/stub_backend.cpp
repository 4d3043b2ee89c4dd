// stub_backend.cpp — a CPU stand-in for libkaldi_fp16 under the host layer.
//
// The host layer (kaldi-fp16_amd/host) is pure orchestration: what it does is the ordered
// sequence of C-ABI calls it makes and their arguments. Every bridge_* / kf_* / ops_* symbol
// the host sources reference is defined here; each appends one text line to stdout and
// returns success. Device memory is a bump allocator over a fake address range (never
// dereferenced), so a pointer prints as "a<allocation index>+<offset>", and streams and
// events are small integer handles. Single-threaded by construction: the call order is
// the order of the lines. kf_dp_* comes from the real csrc/dp.cpp (for kf_dp_plan); the
// few HIP entry points that file references are defined at the bottom and never called,
// because no communicator is bound. The small int32 tables the host uploads
// (bridge_transfer_int32) are kept beside their fake address, so a kernel entry that takes
// only the device copy of a table (kf_update_maxchange) can print it.
#include <cinttypes>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/bridge.h"
#include "../../include/kf_ops.h"
#include "../../include/ops.h"

namespace {

struct Alloc {
    uintptr_t base;
    size_t size;
};
const uintptr_t kBase = (uintptr_t)1 << 44;
std::vector<Alloc> g_allocs;
uintptr_t g_next = kBase;
uintptr_t g_stream = 0;       // current stream handle (0 = the default stream)
int g_nstreams = 0, g_nevents = 0, g_wgrad_target = 512;
std::map<uintptr_t, std::vector<int32_t>> g_tables;  // what bridge_transfer_int32 uploaded, by address

std::string P(const void *p) {
    if (!p) return "null";
    const uintptr_t v = (uintptr_t)p;
    if (v < kBase || v >= g_next) return "host";
    // allocations are in address order with a gap between them; one-past-the-end belongs
    size_t lo = 0, hi = g_allocs.size();
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        (g_allocs[mid].base <= v ? lo : hi) = mid;
    }
    if (g_allocs.empty() || v > g_allocs[lo].base + g_allocs[lo].size) return "host";
    char b[64];
    snprintf(b, sizeof b, "a%zu+%zu", lo, (size_t)(v - g_allocs[lo].base));
    return b;
}
std::string S(const void *s) { return "s" + std::to_string((uintptr_t)s); }
std::string Ev(const void *e) { return "e" + std::to_string((uintptr_t)e); }
std::string ints(const int *v, int n) {
    if (!v) return "null";
    std::string s = "[";
    for (int i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s + "]";
}
// one trace line: the call, then the stream current at the call
void line(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vprintf(fmt, ap);
    va_end(ap);
    printf(" @s%" PRIuPTR "\n", g_stream);
}
std::string opnd(const KfOperand *o) {
    if (!o) return "null";
    const int np = o->nparts < 0 ? 0 : o->nparts > KF_MAX_PARTS ? KF_MAX_PARTS : o->nparts;
    char b[512];
    snprintf(b, sizeof b,
             "{base=%s ld=%lld nrows=%d ncols=%d kcontig=%d nparts=%d part_width=%d T=%d hout=%d hsrc=%d "
             "hmul=%d hdiv=%d tpolicy=%d dt=%s dh=%s edge_t=%s edge_row=%s fmt=%d scales=%s lds=%lld mask=%s "
             "mask_rows=%d tmul=%d t0=%d}",
             P(o->base).c_str(), o->ld, o->nrows, o->ncols, o->kcontig, o->nparts, o->part_width, o->T, o->hout,
             o->hsrc, o->hmul, o->hdiv, o->tpolicy, ints(o->dt, np).c_str(), ints(o->dh, np).c_str(),
             ints(o->edge_t, np).c_str(), ints(o->edge_row, np).c_str(), o->fmt, P(o->scales).c_str(), o->lds,
             P(o->mask).c_str(), o->mask_rows, o->tmul, o->t0);
    return b;
}
std::string epi(const KfEpilogue *e) {
    if (!e) return "null";
    char b[768];
    snprintf(b, sizeof b,
             "{out=%s ldo=%lld alpha=%g beta=%g bias=%s relu=%d mask_out=%s scale=%s shift=%s resid=%s ldr=%lld "
             "resid_alpha=%g out2=%s ldo2=%lld scale2=%s mask_in=%s out8=%s ldo8=%lld scale8=%s out8_src=%d "
             "edge_out=%s edge_r0=%d edge_r1=%d edge_src=%d row_group=%d row_stride=%d}",
             P(e->out).c_str(), e->ldo, e->alpha, e->beta, P(e->bias).c_str(), e->relu, P(e->mask_out).c_str(),
             P(e->scale).c_str(), P(e->shift).c_str(), P(e->resid).c_str(), e->ldr, e->resid_alpha,
             P(e->out2).c_str(), e->ldo2, P(e->scale2).c_str(), P(e->mask_in).c_str(), P(e->out8).c_str(), e->ldo8,
             P(e->scale8).c_str(), e->out8_src, P(e->edge_out).c_str(), e->edge_r0, e->edge_r1, e->edge_src,
             e->row_group, e->row_stride);
    if (!e->drop && !e->ld_drop && !e->row_seg) return b;
    // the per-sequence dropout fields, only when one is set
    std::string s(b, strlen(b) - 1);
    snprintf(b, sizeof b, " drop=%s ld_drop=%lld row_seg=%s}", P(e->drop).c_str(), e->ld_drop, P(e->row_seg).c_str());
    return s + b;
}
std::string att(const KfAttention *a) {
    char b[256];
    snprintf(b, sizeof b, "{proj=%s ldp=%lld T=%d heads=%d kd=%d vd=%d ctx=%d left=%d stride=%d key_scale=%g}",
             P(a->proj).c_str(), a->ldp, a->T, a->num_heads, a->key_dim, a->value_dim, a->context, a->num_left,
             a->stride, a->key_scale);
    return b;
}
std::string qjob(const KfQuantJob &j) {
    char b[256];
    snprintf(b, sizeof b, "{src=%s ld=%lld rows=%d cols=%d tr=%d q=%s ldq=%lld s=%s lds=%lld}", P(j.src).c_str(),
             j.ld_src, j.rows, j.cols, j.transpose, P(j.q).c_str(), j.ldq, P(j.scales).c_str(), j.lds);
    return b;
}
// a table of n entries, element by element
template <class T, class F>
std::string table(const T *t, int n, F one) {
    if (!t) return "null";
    std::string s = "[";
    for (int i = 0; i < n; ++i) s += (i ? " " : "") + one(t[i]);
    return s + "]";
}
// a table the kernel reads from device memory: the copy the host uploaded to that address
template <class T, class F>
std::string dev_table(const void *dev, int n, F one) {
    const auto it = g_tables.find((uintptr_t)dev);
    if (it == g_tables.end() || it->second.size() * 4 < (size_t)n * sizeof(T)) return P(dev) + "(not uploaded)";
    std::vector<T> t((size_t)n);
    memcpy(t.data(), it->second.data(), (size_t)n * sizeof(T));
    return P(dev) + "=" + table(t.data(), n, one);
}
std::string fmt(const char *f, ...) {
    char b[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}
std::string seg(const KfUpdSegment &g) { return fmt("{%lld..%lld comp=%d wg=%d}", g.begin, g.end, g.comp, g.first_wg); }
std::string ucomp(const KfUpdComp &c) {
    return fmt("{max_change=%g l2=%g lr_factor=%g wg=%d+%d}", c.max_change, c.l2, c.lr_factor, c.first_wg, c.num_wg);
}
std::string omat(const KfOrthoMat &m) { return fmt("{off=%lld K=%d n=%d c=%g}", m.offset, m.K, m.n, m.c); }
std::string ngpre(const KfNgPre &p) {
    return fmt("{D=%d R=%d w=%lld h=%lld s=%lld st=%lld}", p.D, p.R, p.w_off, p.h_off, p.s_off, p.st_off);
}
std::string ngcomp(const KfNgComp &c) {
    return fmt("{dw=%lld db=%lld K=%d N=%d in=%d out=%d}", c.dw_off, c.db_off, c.K, c.N, c.pre_in, c.pre_out);
}
std::string ngopts(const KfNgOpts *o) {
    if (!o) return "null";
    return fmt("{rank_in=%d rank_out=%d period=%d history=%g alpha=%g eps=%g delta=%g}", o->rank_in, o->rank_out,
               o->update_period, o->num_samples_history, o->alpha, o->epsilon, o->delta);
}
std::string dlayer(const KfDropLayer &d) {
    return fmt("{mask=%s ld=%lld dim=%d ord=%d p=%g}", P(d.mask).c_str(), d.ld, d.dim, d.ordinal, d.p);
}

}  // namespace

// the driver starts every scenario from the same allocator and handle state, so a
// scenario's trace does not depend on the ones before it
extern "C" void stub_reset(void) {
    g_allocs.clear();
    g_next = kBase;
    g_stream = 0;
    g_nstreams = g_nevents = 0;
    g_wgrad_target = 512;
    g_tables.clear();
}

extern "C" {

// ---- bridge ----
const char *bridge_last_error(void) { return nullptr; }
int bridge_gpu_sync(void) {
    line("bridge_gpu_sync");
    return 0;
}
void *bridge_gpu_malloc(size_t bytes) {
    g_allocs.push_back(Alloc{g_next, bytes});
    void *p = (void *)g_next;
    g_next = (g_next + bytes + 256 + 255) / 256 * 256;  // 256-byte aligned, a gap after each
    line("bridge_gpu_malloc %zu -> %s", bytes, P(p).c_str());
    return p;
}
void bridge_gpu_free(void *ptr) { line("bridge_gpu_free %s", P(ptr).c_str()); }
void bridge_gpu_memset(void *ptr, int value, size_t bytes) { line("bridge_gpu_memset %s %d %zu", P(ptr).c_str(), value, bytes); }
int bridge_transfer_fp16(void *dst, const uint16_t *, size_t count) {
    line("bridge_transfer_fp16 %s %zu", P(dst).c_str(), count);
    return 0;
}
int bridge_transfer_int32(void *dst, const int32_t *src, size_t count) {
    line("bridge_transfer_int32 %s %zu", P(dst).c_str(), count);
    g_tables[(uintptr_t)dst].assign(src, src + count);
    return 0;
}
int bridge_transfer_float32(void *dst, const float *, size_t count) {
    line("bridge_transfer_float32 %s %zu", P(dst).c_str(), count);
    return 0;
}
int bridge_read_fp16(uint16_t *dst, const void *src, size_t count) {
    line("bridge_read_fp16 %s %zu", P(src).c_str(), count);
    memset(dst, 0, count * 2);
    return 0;
}

// ---- ops ----
const char *ops_last_error(void) { return nullptr; }
int ops_log_softmax(void *data, int rows, int cols) {
    line("ops_log_softmax %s %d %d", P(data).c_str(), rows, cols);
    return 0;
}
int ops_copy(void *dst, const void *src, int count) {
    line("ops_copy %s %s %d", P(dst).c_str(), P(src).c_str(), count);
    return 0;
}
int ops_combine_feature_maps(void *data, int T, int total_dim, int height, int nf1, int nf2) {
    line("ops_combine_feature_maps %s %d %d %d %d %d", P(data).c_str(), T, total_dim, height, nf1, nf2);
    return 0;
}

// ---- streams, events, errors ----
void kf_set_stream(void *s) {
    line("kf_set_stream %s", S(s).c_str());
    g_stream = (uintptr_t)s;
}
void *kf_get_stream(void) {
    line("kf_get_stream");
    return (void *)g_stream;
}
void *kf_stream_new(void) {
    void *s = (void *)(uintptr_t)++g_nstreams;
    line("kf_stream_new -> %s", S(s).c_str());
    return s;
}
void *kf_stream_new_high(void) {
    void *s = (void *)(uintptr_t)++g_nstreams;
    line("kf_stream_new_high -> %s", S(s).c_str());
    return s;
}
void kf_stream_free(void *s) { line("kf_stream_free %s", S(s).c_str()); }
void *kf_event_new(void) {
    void *e = (void *)(uintptr_t)++g_nevents;
    line("kf_event_new -> %s", Ev(e).c_str());
    return e;
}
void kf_event_free(void *e) { line("kf_event_free %s", Ev(e).c_str()); }
int kf_event_record(void *e, void *s) {
    line("kf_event_record %s %s", Ev(e).c_str(), S(s).c_str());
    return 0;
}
int kf_stream_wait(void *s, void *e) {
    line("kf_stream_wait %s %s", S(s).c_str(), Ev(e).c_str());
    return 0;
}
const char *kf_last_error(void) { return nullptr; }
const char *kf_layers_last_error(void) { return nullptr; }
int kf_take_pending(const char *where) {
    line("kf_take_pending %s", where ? where : "null");
    return 0;
}
int kf_debug_spin(void *stream, long long cycles) {
    line("kf_debug_spin %s %lld", S(stream).c_str(), cycles);
    return 0;
}

// ---- GEMMs ----
int kf_gemm_fused(int M, int N, int K, const KfOperand *A, const KfOperand *B, const KfEpilogue *E) {
    line("kf_gemm_fused %d %d %d A=%s B=%s E=%s", M, N, K, opnd(A).c_str(), opnd(B).c_str(), epi(E).c_str());
    return 0;
}
int kf_gemm_fused_edge(int M, int N, int K, const KfOperand *A, const KfOperand *B, const KfEpilogue *E,
                       void *edge_out, const void *x0, const void *x1, const void *W, int cols) {
    line("kf_gemm_fused_edge %d %d %d A=%s B=%s E=%s edge_out=%s x0=%s x1=%s W=%s cols=%d", M, N, K, opnd(A).c_str(),
         opnd(B).c_str(), epi(E).c_str(), P(edge_out).c_str(), P(x0).c_str(), P(x1).c_str(), P(W).c_str(), cols);
    return 0;
}
int kf_gemm_wgrad(int M, int N, int K, const KfOperand *A, const KfOperand *B, float *dW, long long ldw,
                  float *bias_grad, int accumulate) {
    line("kf_gemm_wgrad %d %d %d A=%s B=%s dW=%s ldw=%lld db=%s acc=%d", M, N, K, opnd(A).c_str(), opnd(B).c_str(),
         P(dW).c_str(), ldw, P(bias_grad).c_str(), accumulate);
    return 0;
}
int kf_gemm_wgrad_scaled(int M, int N, int K, const KfOperand *A, const KfOperand *B, float *dW, long long ldw,
                         float *bias_grad, int accumulate, const float *col_scale) {
    line("kf_gemm_wgrad_scaled %d %d %d A=%s B=%s dW=%s ldw=%lld db=%s acc=%d col_scale=%s", M, N, K,
         opnd(A).c_str(), opnd(B).c_str(), P(dW).c_str(), ldw, P(bias_grad).c_str(), accumulate, P(col_scale).c_str());
    return 0;
}
int kf_gemm_wgrad_target(int wgs) {
    const int old = g_wgrad_target;
    if (wgs > 0) g_wgrad_target = wgs;
    line("kf_gemm_wgrad_target %d -> %d", wgs, old);
    return old;
}
int kf_quant_mxfp8(const void *src, long long ld_src, int rows, int cols, int transpose, void *q, long long ldq,
                   uint8_t *scales, long long lds) {
    line("kf_quant_mxfp8 %s", qjob(KfQuantJob{src, ld_src, rows, cols, transpose, q, ldq, scales, lds}).c_str());
    return 0;
}
int kf_quant_mxfp8_batch(int n, const KfQuantJob *jobs) {
    std::string s;
    for (int i = 0; i < n; ++i) s += " " + qjob(jobs[i]);
    line("kf_quant_mxfp8_batch %d%s", n, s.c_str());
    return 0;
}
int kf_transpose_batch(int n, const void *const *src, void *const *dst, const int *M, const int *N) {
    std::string s;
    for (int i = 0; i < n; ++i)
        s += " {" + P(src[i]) + " -> " + P(dst[i]) + " " + std::to_string(M[i]) + "x" + std::to_string(N[i]) + "}";
    line("kf_transpose_batch %d%s", n, s.c_str());
    return 0;
}
int kf_rows_sum_mask(void *edge, const void *src, long long ld, int r0, int r1, int cols, const uint8_t *mask) {
    line("kf_rows_sum_mask %s %s %lld %d %d %d %s", P(edge).c_str(), P(src).c_str(), ld, r0, r1, cols, P(mask).c_str());
    return 0;
}
int kf_rows_sum_list(void *edge, const void *src, long long ld, const int *rows, int n, int cols) {
    line("kf_rows_sum_list %s %s %lld %s %d", P(edge).c_str(), P(src).c_str(), ld, ints(rows, n).c_str(), cols);
    return 0;
}

// ---- layer pieces ----
int kf_small_gemm(const void *x, int ldx, const void *M, void *y, int ldy, int T, int K, int N) {
    line("kf_small_gemm %s %d %s %s %d %d %d %d", P(x).c_str(), ldx, P(M).c_str(), P(y).c_str(), ldy, T, K, N);
    return 0;
}
int kf_bn_apply(const void *x, void *y, long long rows, int D, const float *scale, const float *shift) {
    line("kf_bn_apply %s %s %lld %d %s %s", P(x).c_str(), P(y).c_str(), rows, D, P(scale).c_str(), P(shift).c_str());
    return 0;
}
int kf_conv_c1_forward(int T, int hin, int hout, int sub, int fout, int noff, const int *dt, const int *dh,
                       const void *x, const void *W, const void *bias, const float *scale, const float *shift, void *y,
                       uint8_t *mask) {
    line("kf_conv_c1_forward %d %d %d %d %d %d dt=%s dh=%s x=%s W=%s bias=%s scale=%s shift=%s y=%s mask=%s", T, hin,
         hout, sub, fout, noff, ints(dt, noff).c_str(), ints(dh, noff).c_str(), P(x).c_str(), P(W).c_str(),
         P(bias).c_str(), P(scale).c_str(), P(shift).c_str(), P(y).c_str(), P(mask).c_str());
    return 0;
}
int kf_conv_c1_wgrad(int T, int hin, int hout, int sub, int fout, int noff, const int *dt, const int *dh,
                     const void *x, const void *dz, float *dW, float *db) {
    line("kf_conv_c1_wgrad %d %d %d %d %d %d dt=%s dh=%s x=%s dz=%s dW=%s db=%s", T, hin, hout, sub, fout, noff,
         ints(dt, noff).c_str(), ints(dh, noff).c_str(), P(x).c_str(), P(dz).c_str(), P(dW).c_str(), P(db).c_str());
    return 0;
}
int kf_sgd_flat(float *w32, void *w16, const float *g, float *v, float lr, float mom, long long n) {
    line("kf_sgd_flat %s %s %s %s %g %g %lld", P(w32).c_str(), P(w16).c_str(), P(g).c_str(), P(v).c_str(), lr, mom, n);
    return 0;
}
int kf_gather_rows(void *dst, const void *src, long long row_bytes, int T, int tc0, int tc) {
    line("kf_gather_rows %s %s %lld %d %d %d", P(dst).c_str(), P(src).c_str(), row_bytes, T, tc0, tc);
    return 0;
}
int kf_scatter_rows(void *dst, const void *src, long long row_bytes, int T, int tc0, int tc) {
    line("kf_scatter_rows %s %s %lld %d %d %d", P(dst).c_str(), P(src).c_str(), row_bytes, T, tc0, tc);
    return 0;
}
int kf_scatter_rows_from(void *dst, const void *src, long long row_bytes, int T, int tc0, int tc, int r0) {
    line("kf_scatter_rows_from %s %s %lld %d %d %d %d", P(dst).c_str(), P(src).c_str(), row_bytes, T, tc0, tc, r0);
    return 0;
}
int kf_attention_forward(const KfAttention *a, void *out, long long ldo, uint8_t *mask, const float *scale,
                         const float *shift) {
    line("kf_attention_forward %s %s %lld %s %s %s", att(a).c_str(), P(out).c_str(), ldo, P(mask).c_str(),
         P(scale).c_str(), P(shift).c_str());
    return 0;
}
int kf_attention_backward(const KfAttention *a, const void *dz, long long ldz, void *dproj, float *scratch) {
    line("kf_attention_backward %s %s %lld %s %s", att(a).c_str(), P(dz).c_str(), ldz, P(dproj).c_str(),
         P(scratch).c_str());
    return 0;
}
int kf_combine_feature_maps(const void *a, long long lda, const void *b, long long ldb, const int *dev_seq_off, int B,
                            void *out, long long ldo, int T, int height, int nf1, int nf2) {
    line("kf_combine_feature_maps %s %lld %s %lld %s %d %s %lld %d %d %d %d", P(a).c_str(), lda, P(b).c_str(), ldb,
         P(dev_seq_off).c_str(), B, P(out).c_str(), ldo, T, height, nf1, nf2);
    return 0;
}
int kf_combine_feature_maps_backward(const void *dy, long long ldy, const int *dev_seq_off, int B, void *db,
                                     long long ldb, int height, int nf1, int nf2) {
    line("kf_combine_feature_maps_backward %s %lld %s %d %s %lld %d %d %d", P(dy).c_str(), ldy, P(dev_seq_off).c_str(),
         B, P(db).c_str(), ldb, height, nf1, nf2);
    return 0;
}
int kf_im2col_small(const void *x, long long ldx, int T, int hin, int hout, int sub, int fin, int ntaps, const int *dt,
                    const int *dh, void *Pm, int kp) {
    line("kf_im2col_small %s %lld %d %d %d %d %d %d dt=%s dh=%s %s %d", P(x).c_str(), ldx, T, hin, hout, sub, fin,
         ntaps, ints(dt, ntaps).c_str(), ints(dh, ntaps).c_str(), P(Pm).c_str(), kp);
    return 0;
}
int kf_col2im_small(const void *dP, int T, int hin, int hout, int sub, int fin, int ntaps, const int *dt,
                    const int *dh, int kp, void *dx, long long ldx) {
    line("kf_col2im_small %s %d %d %d %d %d %d dt=%s dh=%s %d %s %lld", P(dP).c_str(), T, hin, hout, sub, fin, ntaps,
         ints(dt, ntaps).c_str(), ints(dh, ntaps).c_str(), kp, P(dx).c_str(), ldx);
    return 0;
}
int kf_rows_gemm(const void *x, long long ldx, const void *W, long long ldw, void *y, long long ldy, int R, int K,
                 int N) {
    line("kf_rows_gemm %s %lld %s %lld %s %lld %d %d %d", P(x).c_str(), ldx, P(W).c_str(), ldw, P(y).c_str(), ldy, R,
         K, N);
    return 0;
}
int kf_rows_wgrad(const void *x, long long ldx, const void *g, long long ldg, float *dW, long long ldd, int R, int M,
                  int N) {
    line("kf_rows_wgrad %s %lld %s %lld %s %lld %d %d %d", P(x).c_str(), ldx, P(g).c_str(), ldg, P(dW).c_str(), ldd,
         R, M, N);
    return 0;
}
int kf_scale_cols(const void *x, long long ldx, const float *scale, void *y, long long ldy, int rows, int cols) {
    line("kf_scale_cols %s %lld %s %s %lld %d %d", P(x).c_str(), ldx, P(scale).c_str(), P(y).c_str(), ldy, rows, cols);
    return 0;
}

// ---- Kaldi-style update, orthonormal constraint ----
long long kf_update_scratch_bytes(long long n, int nseg, int ncomp) {
    const long long b = 256 * (n / KF_UPD_CHUNK + nseg + 2 * (long long)ncomp + 3);
    line("kf_update_scratch_bytes %lld %d %d -> %lld", n, nseg, ncomp, b);
    return b;
}
int kf_update_maxchange(float *w32, void *w16, const float *g, float *v, long long n, const KfUpdSegment *segments,
                        int nseg, const KfUpdComp *comps, int ncomp, float lr, float momentum, float max_param_change,
                        float l2_scale, void *scratch, float *stats) {
    line("kf_update_maxchange %s %s %s %s %lld segs=%s comps=%s lr=%g mom=%g max_param_change=%g l2_scale=%g "
         "scratch=%s stats=%s",
         P(w32).c_str(), P(w16).c_str(), P(g).c_str(), P(v).c_str(), n, dev_table<KfUpdSegment>(segments, nseg, seg).c_str(),
         dev_table<KfUpdComp>(comps, ncomp, ucomp).c_str(), lr, momentum, max_param_change, l2_scale, P(scratch).c_str(),
         P(stats).c_str());
    return 0;
}
long long kf_orthonormal_scratch_bytes(const KfOrthoMat *mats, int nmat) {
    long long b = 256;
    for (int i = 0; i < nmat; ++i) b += 4ll * mats[i].n * mats[i].n * ((mats[i].K + KF_ORTHO_KCHUNK - 1) / KF_ORTHO_KCHUNK + 1);
    line("kf_orthonormal_scratch_bytes %s -> %lld", table(mats, nmat, omat).c_str(), b);
    return b;
}
int kf_orthonormal_constrain(float *w32, void *w16, long long n_params, const KfOrthoMat *mats, const KfOrthoMat *mats_dev,
                             int nmat, void *scratch, float *stats) {
    line("kf_orthonormal_constrain %s %s %lld mats=%s dev=%s scratch=%s stats=%s", P(w32).c_str(), P(w16).c_str(), n_params,
         table(mats, nmat, omat).c_str(), P(mats_dev).c_str(), P(scratch).c_str(), P(stats).c_str());
    return 0;
}

// ---- natural gradient ----
void kf_ng_default_opts(KfNgOpts *o) {  // Kaldi's defaults, as csrc/natgrad.hip
    line("kf_ng_default_opts");
    if (!o) return;
    o->rank_in = 20;
    o->rank_out = 80;
    o->update_period = 4;
    o->num_samples_history = 2000.f;
    o->alpha = 4.f;
    o->epsilon = 1e-10f;
    o->delta = 5e-4f;
}
int kf_ng_init(const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const KfNgOpts *opts, float *w32, void *w16,
               double *sc) {
    line("kf_ng_init pres=%s dev=%s opts=%s %s %s %s", table(pres, npre, ngpre).c_str(), P(pres_dev).c_str(),
         ngopts(opts).c_str(), P(w32).c_str(), P(w16).c_str(), P(sc).c_str());
    return 0;
}
int kf_ng_trx(const KfOperand *op, int ones, float *out) {
    line("kf_ng_trx %s ones=%d %s", opnd(op).c_str(), ones, P(out).c_str());
    return 0;
}
int kf_ng_scales(const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const KfNgOpts *opts, const double *sc,
                 const float *stat, float *report) {
    line("kf_ng_scales pres=%s dev=%s opts=%s %s %s %s", table(pres, npre, ngpre).c_str(), P(pres_dev).c_str(),
         ngopts(opts).c_str(), P(sc).c_str(), P(stat).c_str(), P(report).c_str());
    return 0;
}
long long kf_ng_apply_scratch_bytes(const KfNgComp *comps, int ncomp, const KfNgPre *pres, int npre) {
    long long b = 256;
    for (int i = 0; i < ncomp; ++i) b += 4ll * KF_NG_MAX_RANK * (comps[i].K + 1 + comps[i].N);
    line("kf_ng_apply_scratch_bytes comps=%s pres=%s -> %lld", table(comps, ncomp, ngcomp).c_str(),
         table(pres, npre, ngpre).c_str(), b);
    return b;
}
int kf_ng_apply(float *g, long long n_grad, const KfNgComp *comps, const KfNgComp *comps_dev, int ncomp, const KfNgPre *pres,
                const KfNgPre *pres_dev, int npre, const float *w32, const float *report, void *scratch) {
    line("kf_ng_apply %s %lld comps=%s dev=%s pres=%s dev=%s %s %s %s", P(g).c_str(), n_grad,
         table(comps, ncomp, ngcomp).c_str(), P(comps_dev).c_str(), table(pres, npre, ngpre).c_str(), P(pres_dev).c_str(),
         P(w32).c_str(), P(report).c_str(), P(scratch).c_str());
    return 0;
}
long long kf_ng_state_scratch_bytes(const KfNgPre *pres, int npre) {
    const long long b = 256 + 1024ll * npre;
    line("kf_ng_state_scratch_bytes pres=%s -> %lld", table(pres, npre, ngpre).c_str(), b);
    return b;
}
int kf_ng_state(const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const KfNgOpts *opts, int update, float *w32,
                void *w16, double *sc, const float *stat, void *scratch, float *report) {
    line("kf_ng_state pres=%s dev=%s opts=%s update=%d %s %s %s %s %s %s", table(pres, npre, ngpre).c_str(),
         P(pres_dev).c_str(), ngopts(opts).c_str(), update, P(w32).c_str(), P(w16).c_str(), P(sc).c_str(), P(stat).c_str(),
         P(scratch).c_str(), P(report).c_str());
    return 0;
}

// ---- dropout, SpecAugment, training-mode BatchNorm ----
int kf_dropout_masks(int n, const KfDropLayer *layers, int B, unsigned long long seed, long long step) {
    line("kf_dropout_masks %s B=%d seed=%llu step=%lld", table(layers, n, dlayer).c_str(), B, seed, step);
    return 0;
}
int kf_row_seg(int32_t *row_seg, const int *dev_seq_off, int B, int T, int tc0, int tc) {
    line("kf_row_seg %s %s %d %d %d %d", P(row_seg).c_str(), P(dev_seq_off).c_str(), B, T, tc0, tc);
    return 0;
}
int kf_specaug_rows(int32_t *row_band, const int *dev_seq_off, int B, int T, int dim, int max_bins, float z, int max_zeroed,
                    int max_kept, unsigned ordinal, unsigned long long seed, long long step) {
    line("kf_specaug_rows %s %s %d %d dim=%d max_bins=%d z=%g max_zeroed=%d max_kept=%d ord=%u seed=%llu step=%lld",
         P(row_band).c_str(), P(dev_seq_off).c_str(), B, T, dim, max_bins, z, max_zeroed, max_kept, ordinal, seed, step);
    return 0;
}
int kf_specaug_apply(const void *x, long long ldx, void *y, long long ldy, long long rows, int dim, const int32_t *row_band) {
    line("kf_specaug_apply %s %lld %s %lld %lld %d %s", P(x).c_str(), ldx, P(y).c_str(), ldy, rows, dim, P(row_band).c_str());
    return 0;
}
int kf_bn_train_stats(const void *r, long long ld, int rows, int D, float eps, float target_rms, float *mean, float *var,
                      float *scale, float *shift, double *acc_count, double *acc_sum, double *acc_sumsq) {
    line("kf_bn_train_stats %s %lld %d %d eps=%g rms=%g %s %s %s %s acc=%s %s %s", P(r).c_str(), ld, rows, D, eps, target_rms,
         P(mean).c_str(), P(var).c_str(), P(scale).c_str(), P(shift).c_str(), P(acc_count).c_str(), P(acc_sum).c_str(),
         P(acc_sumsq).c_str());
    return 0;
}
int kf_bn_train_apply(const void *r, long long ld, int rows, int D, const float *scale, const float *shift, const float *drop,
                      long long ld_drop, const int32_t *row_seg, const void *resid, long long ldr, float alpha, void *out,
                      long long ldo) {
    line("kf_bn_train_apply %s %lld %d %d %s %s drop=%s %lld %s resid=%s %lld alpha=%g out=%s %lld", P(r).c_str(), ld, rows, D,
         P(scale).c_str(), P(shift).c_str(), P(drop).c_str(), ld_drop, P(row_seg).c_str(), P(resid).c_str(), ldr, alpha,
         P(out).c_str(), ldo);
    return 0;
}
int kf_bn_train_bwd_stats(const void *g, long long ldg, const void *r, long long ldr, int rows, int D, const float *scale,
                          const float *shift, float target_rms, const float *drop, long long ld_drop, const int32_t *row_seg,
                          float *a, float *b) {
    line("kf_bn_train_bwd_stats %s %lld %s %lld %d %d %s %s rms=%g drop=%s %lld %s a=%s b=%s", P(g).c_str(), ldg, P(r).c_str(),
         ldr, rows, D, P(scale).c_str(), P(shift).c_str(), target_rms, P(drop).c_str(), ld_drop, P(row_seg).c_str(),
         P(a).c_str(), P(b).c_str());
    return 0;
}
int kf_bn_train_bwd_apply(const void *g, long long ldg, const void *r, long long ldr, int rows, int D, const float *scale,
                          const float *shift, float target_rms, const float *a, const float *b, const float *drop,
                          long long ld_drop, const int32_t *row_seg, const uint8_t *mask, long long ld_mask, void *dz,
                          long long lddz) {
    line("kf_bn_train_bwd_apply %s %lld %s %lld %d %d %s %s rms=%g a=%s b=%s drop=%s %lld %s mask=%s %lld dz=%s %lld",
         P(g).c_str(), ldg, P(r).c_str(), ldr, rows, D, P(scale).c_str(), P(shift).c_str(), target_rms, P(a).c_str(),
         P(b).c_str(), P(drop).c_str(), ld_drop, P(row_seg).c_str(), P(mask).c_str(), ld_mask, P(dz).c_str(), lddz);
    return 0;
}

}  // extern "C"

// ---- what csrc/dp.cpp references: two C++ symbols of libkaldi_fp16 and a few HIP entry
// points. No communicator is bound, so none is ever called. ----
struct ihipStream_t;
ihipStream_t *kf_stream() { return nullptr; }
int kf_dp_debug_mean_launch(float *, const float *, size_t, ihipStream_t *) { return -1; }

extern "C" {
#define HIP_NEVER(name) \
    int name(...) { return 1; }
HIP_NEVER(hipDeviceGetStreamPriorityRange)
HIP_NEVER(hipEventCreateWithFlags)
HIP_NEVER(hipEventDestroy)
HIP_NEVER(hipEventRecord)
HIP_NEVER(hipGetLastError)
HIP_NEVER(hipMemcpyAsync)
HIP_NEVER(hipSetDevice)
HIP_NEVER(hipStreamCreateWithPriority)
HIP_NEVER(hipStreamDestroy)
HIP_NEVER(hipStreamSynchronize)
HIP_NEVER(hipStreamWaitEvent)
const char *hipGetErrorString(int) { return "stub"; }

}  // extern "C"
