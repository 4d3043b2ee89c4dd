/*
 * kf_ops.h — MI355X extension of the kaldi-fp16 C-ABI: fused, implicitly
 * addressed FP16 MFMA GEMMs and the few multi-tensor kernels the CNN-TDNN
 * training step needs. Nothing here replaces a reference symbol; these entry
 * points are what this build's host layer (the C++ mirror of internal/nnet and
 * internal/gpu, see kf_nnet.h) calls so that the splice / im2col / epilogue
 * work the reference does as separate kernels and host round trips
 * (internal/nnet/forward.go:418-790, internal/gpu/backward_ops.go:162-253)
 * happens inside one GEMM launch. Plain C types only; no torch, no HIP types.
 *
 * Operand addressing (KfOperand). An operand is a logical row-major matrix
 * Op[r][c] (r < nrows, c < ncols) whose 8-element column chunks are fetched
 * from memory by this rule (all counts in elements):
 *   part p = c / part_width, kk = c % part_width      (nparts parts)
 *   t = r / hout, h = r % hout                         (hout = 1 for TDNN rows)
 *   if edge_t[p] >= 0 and t == edge_t[p]: st = edge_row[p] (a spare row of the
 *      same buffer, e.g. row T, holding a precomputed sum; no range checks)
 *   else st = t + dt[p]; outside [0, T): clamp (tpolicy=KF_CLAMP) or zero (KF_ZERO)
 *   shn = h*hmul + dh[p]; zero unless shn % hdiv == 0; sh = shn / hdiv,
 *   zero unless 0 <= sh < hsrc
 *   value = base[st*ld + sh*part_width + kk]
 * With nparts=1, hout=1, dt=0 this is a plain [nrows x ncols] matrix with
 * leading dimension ld. The same rule expresses the TDNN time splice
 * (forward.go:699-790: dt = {-s, 0} clamp, or {0, +s} clamp), the conv im2col
 * (forward.go:435-456: dt x dh cross product, hmul = subsample, zero pad),
 * and their transposes used by the input-gradient GEMMs.
 *
 * Orientation: an operand is "k-contiguous" when its columns run along the
 * GEMM reduction index (row-major A[M][K], or B stored [N][K]); otherwise its
 * rows run along the reduction (A stored [K][M], B stored [K][N]).
 *
 * MXFP8 operands (fmt = KF_FMT_MXFP8, the OCP microscaling format): elements are
 * OCP e4m3 bytes and every 32 consecutive elements of a source row share one
 * E8M0 scale byte (value 2^(byte-127)) at scales[st*lds + c/32], st and c the
 * source row and column of the rule above. Only k-contiguous operands with
 * hout = 1 are accepted, ncols and part_width multiples of 128, ld multiple of
 * 16; both operands of a GEMM must then be MXFP8 (kf_gemm_fused runs the CDNA4
 * v_mfma_scale_f32_16x16x128_f8f6f4, twice the fp16 MFMA rate).
 *
 * Masked operands (mask != NULL, fp16 only): with i = st*ld + sh*part_width + kk the
 * linear source index of the rule above, the element reads as zero unless bit i of mask
 * (bit i % 8 of byte i / 8) is set; rows st >= mask_rows (e.g. an edge row) are not
 * masked. This is how the TDNN-F backward reads dz = g * bnscale * relu_mask without
 * storing it: g with the forward's ReLU mask, the BN scale folded into the other operand
 * (kf_scale_cols on W2) or into the weight gradient (kf_gemm_wgrad_scaled). Accepted on the A
 * operand of kf_gemm_fused (k-contiguous plain or two-part time splice, N = 160 / 320,
 * k-contiguous B) and the B operand of kf_gemm_wgrad(_scaled) (plain, reduction-major).
 */
#ifndef KALDI_FP16_AMD_KF_OPS_H
#define KALDI_FP16_AMD_KF_OPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KF_MAX_PARTS 9
#define KF_ZERO 0
#define KF_CLAMP 1

typedef struct {
    const void *base;  /* fp16 */
    long long ld;      /* elements between consecutive source rows */
    int nrows, ncols;  /* logical shape of Op */
    int kcontig;       /* 1: columns are the reduction index */
    int nparts, part_width;
    int T, hout, hsrc, hmul, hdiv, tpolicy;
    int dt[KF_MAX_PARTS];
    int dh[KF_MAX_PARTS];
    int edge_t[KF_MAX_PARTS];
    int edge_row[KF_MAX_PARTS];
    int fmt;                   /* KF_FMT_FP16 (0) or KF_FMT_MXFP8 (1) */
    const uint8_t *scales;     /* MXFP8: E8M0 block scales */
    long long lds;             /* MXFP8: bytes between the scale rows of consecutive source rows */
    const uint8_t *mask;       /* masked operand (above), or NULL */
    int mask_rows;             /* source rows the mask covers */
    /* time-strided rows (a conv evaluated on a subset of its output frames, the row-
     * subsampled step's last conv): st = t0 + t*tmul + dt[p] in the rule above. 0 / 0 =
     * the plain rule. Only the A operand of a convolution that runs on a halo kernel takes
     * it: kf_gemm_fused's im2col operand (forward) and kf_gemm_wgrad's (weight gradient over
     * the strided output frames); other uses fail. */
    int tmul, t0;
} KfOperand;

#define KF_FMT_FP16 0
#define KF_FMT_MXFP8 1

/*
 * Fused epilogue, applied per output element (m, n) to the fp32 accumulator:
 *   v = alpha*acc (+ beta*out[m][n]) (+ bias[n])
 *   if relu: mask_out bit (m*ldo+n) = v > 0; v = max(v, 0)
 *   if scale: v = v*scale[n] + shift[n]          (frozen BatchNorm, folded)
 *   if drop and scale: v *= drop[row_seg[m]][n]   (per-sequence dropout mask, below)
 *   if resid: v += resid_alpha * resid[m][n]     (TDNN-F bypass / grad bypass)
 *   out[m][n] = rne_fp16(v)                       (when out != NULL)
 *   if out2: out2[m][n] = rne_fp16(v * scale2[n] * bit(mask_in, m*ldo2+n)), with drop and
 *            out2: rne_fp16((v * scale2[n]) * drop[row_seg[m]][n] * bit(mask_in, m*ldo2+n))
 *   if out8: MXFP8 copy (kf_quant_mxfp8's rule, 32-column blocks) of the unrounded v, or
 *            with out8_src = 1 of the unrounded out2 value
 *   if edge_out: edge_out[n] = rne_fp16(sum over rows m in [edge_r0, edge_r1) of the stored
 *            out[m][n] (edge_src = 0) or out2[m][n] (edge_src = 1)), in row order: kf_rows_sum
 *            of the result, written by the workgroups of the row tile holding those rows (a
 *            separate sum kernel after the GEMM when the rows span two tiles)
 * Masks are bit-packed in the linear element order of the tensor they describe
 * (bit i of byte i/8), so producer and consumer may tile differently.
 * drop: a column factor per row segment, Kaldi's GeneralDropoutComponent with
 * one mask row per sequence: fp32 [nseg x ld_drop], row_seg[m] the segment of GEMM row m. A
 * launch uses it for one of the two places above, never both: with scale (the forward, after
 * the BatchNorm step and before the bypass) or with out2 (the input gradient's dz). drop with
 * neither or with both, without row_seg, with row_group, out8, beta != 0, a masked or an MXFP8 operand,
 * ld_drop % 8 != 0 or a drop pointer that is not 16-byte aligned fails; so does a product
 * that would run on a tile without the drop variant (it exists for N > 64 other than
 * N = 160 / 320 with a plain or two-part time-spliced A and B, fp16).
 */
typedef struct {
    void *out;
    long long ldo;
    float alpha, beta;
    const void *bias;      /* fp16 [N] or NULL */
    int relu;
    uint8_t *mask_out;     /* or NULL */
    const float *scale;    /* fp32 [N] or NULL */
    const float *shift;    /* fp32 [N] (required with scale) */
    const void *resid;     /* fp16, or NULL */
    long long ldr;
    float resid_alpha;
    void *out2;            /* fp16, or NULL */
    long long ldo2;
    const float *scale2;   /* fp32 [N] or NULL (= 1) */
    const uint8_t *mask_in;/* or NULL (= all ones) */
    void *out8;            /* e4m3 [M x ldo8], or NULL */
    long long ldo8;
    uint8_t *scale8;       /* E8M0 [M x ldo8/32] (required with out8) */
    int out8_src;          /* 0: out8 quantises v (out's value); 1: out2's value (needs out2) */
    void *edge_out;        /* fp16 [N], or NULL: column sums of rows [edge_r0, edge_r1) (above) */
    int edge_r0, edge_r1, edge_src;
    /* grouped output rows: with row_group > 0, GEMM row m addresses row
     * (m / row_group) * row_stride + m % row_group of every row operand above (out, out2,
     * resid, mask_out, mask_in, out8): a transposed conv evaluated on every third frame
     * writes its frames in place. 0 = rows as they are. Not with edge_out. */
    int row_group, row_stride;
    const float *drop;      /* fp32 [nseg x ld_drop] per-segment column factors, or NULL */
    long long ld_drop;
    const int32_t *row_seg; /* [M]: the segment (row of drop) of GEMM row m; required with drop */
} KfEpilogue;

/* current stream for every launch made by this library on the calling thread
 * (NULL = legacy default stream, the reference's behaviour) */
void kf_set_stream(void *hip_stream);
void *kf_get_stream(void);
/* streams and events for host layers built without HIP headers (libkaldi_fp16_nnet's
 * weight-gradient stream): a non-blocking stream (NULL on failure), a timing-disabled
 * event; record / wait return 0 or -1 */
void *kf_stream_new(void);
void *kf_stream_new_high(void);  /* the device's highest stream priority */
void kf_stream_free(void *hip_stream);
void *kf_event_new(void);
void kf_event_free(void *hip_event);
int kf_event_record(void *hip_event, void *hip_stream);
int kf_stream_wait(void *hip_stream, void *hip_event);

/* C[M x N] = epilogue(A . B^T-style contraction over K) */
int kf_gemm_fused(int M, int N, int K, const KfOperand *A, const KfOperand *B,
                  const KfEpilogue *epi);

/*
 * Weight-gradient GEMM with the reduction split over workgroups:
 *   dW[M x N] (fp32, leading dim ldw) (+)= sum_r A(r, m) * B(r, n)
 * bias_grad[N] (fp32, optional) (+)= sum_r B(r, n).
 * accumulate=0 overwrites, 1 adds. Deterministic (slab reduction, no atomics).
 */
int kf_gemm_wgrad(int M, int N, int K, const KfOperand *A, const KfOperand *B, float *dW,
                  long long ldw, float *bias_grad, int accumulate);
/* 1 when kf_gemm_wgrad would run this product on the 3x3 conv halo kernel (the only one that takes
 * time-strided rows, KfOperand.tmul / t0), 0 when it would not, -1 for an invalid operand. No
 * launch and no HIP call: a caller asks before it plans a time-strided weight gradient. */
int kf_gemm_wgrad_halo_applies(int M, int N, int K, const KfOperand *A, const KfOperand *B);
/* kf_gemm_wgrad, then dW[:, n] and bias_grad[n] scaled by col_scale[n] (fp32 [N]) in the
 * split-K reduction: the TDNN-F affine weight gradient on the implicit dz (a masked B
 * operand g with the BN scale applied here) */
int kf_gemm_wgrad_scaled(int M, int N, int K, const KfOperand *A, const KfOperand *B, float *dW,
                         long long ldw, float *bias_grad, int accumulate, const float *col_scale);
/* split-K workgroup target of kf_gemm_wgrad on the calling thread (default 512); returns
 * the previous value (wgs <= 0: query only) */
int kf_gemm_wgrad_target(int wgs);

/*
 * MXFP8 quantisation (OCP MX): per block of 32 consecutive values of a row,
 * amax = max |v|, scale = 2^(floor(log2 amax) - 8) (E8M0 byte = exponent + 127,
 * clamped to [1, 253]; amax = 0 gives byte 127), q = e4m3_rne(clamp(v / scale, +-448)).
 *   transpose = 0: src [rows x cols] fp16 (ld_src); transpose = 1: q row r is
 *   column r of src [cols x rows] (weights W[K][N] -> W8[N][K]).
 * q: [rows x ldq] bytes, scales: [rows][lds]; columns cols .. roundup(cols, 128)-1
 * of q and their scale bytes are written as zero / 127 (padding read by the GEMM).
 */
int kf_quant_mxfp8(const void *src, long long ld_src, int rows, int cols, int transpose,
                   void *q, long long ldq, uint8_t *scales, long long lds);

/* Up to KF_QUANT_MAX kf_quant_mxfp8 calls in one launch (the weight copies after each
 * update: ~80 small matrices per step, each too small to fill the GPU on its own). Same
 * arguments and results as kf_quant_mxfp8, per job. */
#define KF_QUANT_MAX 32
typedef struct KfQuantJob {
    const void *src;
    long long ld_src;
    int rows, cols, transpose;
    void *q;
    long long ldq;
    uint8_t *scales;
    long long lds;
} KfQuantJob;
int kf_quant_mxfp8_batch(int n, const KfQuantJob *jobs);

/* out[j] = rne_fp16(sum_c x0[c] W[j][c] + x1[c] W[rows + j][c]), j < rows, W [2*rows x cols]
 * fp16 row-major, fp32 accumulation; cols % 8 == 0, 16-byte aligned pointers (out is not
 * required to be: it is written per element). One row of a two-part product. */
int kf_dot2_rows(void *out, const void *x0, const void *x1, const void *W, int rows, int cols);
/* kf_gemm_fused of an MXFP8 product (rows 0 .. M-1), whose last row tile's workgroups also
 * compute kf_dot2_rows(edge_out, x0, x1, W, N, cols): the TDNN-F affine input gradient's
 * clamped-edge row T - 1 (M = T - 1) in the same launch. As a separate one-row kernel beside
 * the weight-gradient stream it waited ~340 us per layer for CU slots (3072 model). */
int kf_gemm_fused_edge(int M, int N, int K, const KfOperand *A, const KfOperand *B, const KfEpilogue *epi,
                       void *edge_out, const void *x0, const void *x1, const void *W, int cols);

/* edge[c] = rne_fp16(sum_{r in [r0, r1)} src[r*ld + c]) for c < cols
 * (edge may be a spare row of src's own allocation) */
int kf_rows_sum(void *edge, const void *src, long long ld, int r0, int r1, int cols);
/* the same over the masked source: element r*ld + c counts only when its bit in mask is set */
int kf_rows_sum_mask(void *edge, const void *src, long long ld, int r0, int r1, int cols,
                     const uint8_t *mask);

/* ---- non-MFMA layer pieces (csrc/layers.hip) ---- */
/* y[T x N] = x[T x K] . M[K x N], K <= 64, N % 8 == 0 (IDCT, forward.go:317-330) */
int kf_small_gemm(const void *x, int ldx, const void *M, void *y, int ldy, int T, int K, int N);
/* y = rne(x*scale[d] + shift[d]) on [rows x D] (frozen BatchNorm, folded) */
int kf_bn_apply(const void *x, void *y, long long rows, int D, const float *scale,
                const float *shift);
/* conv-relu-batchnorm with one input filter (im2col K = noff), fused epilogue;
 * y [(T*hout) x fout], mask bits in the same element order */
int kf_conv_c1_forward(int T, int hin, int hout, int sub, int fout, int noff, const int *dt,
                       const int *dh, const void *x, const void *W, const void *bias,
                       const float *scale, const float *shift, void *y, uint8_t *mask);
/* its weight / bias gradient (fp32, overwritten; zeros for T <= 0), deterministic */
int kf_conv_c1_wgrad(int T, int hin, int hout, int sub, int fout, int noff, const int *dt,
                     const int *dh, const void *x, const void *dz, float *dW, float *db);
/* one-launch SGD over a flat parameter set: v = mom*v + g; w32 -= lr*v; w16 = rne(w32) */
int kf_sgd_flat(float *w32, void *w16, const float *g, float *v, float lr, float mom,
                long long n);
int kf_f32_to_f16_flat(const float *src, void *dst, long long n);

/* ---- Kaldi-style parameter update (csrc/update.hip) ----
 * Momentum SGD over a flat parameter set whose elements are grouped into components, with a
 * per-component L2 term and learning-rate factor, each component's step limited to its
 * max-change and the whole step to max_param_change. For element i of component c:
 *   v_i = momentum * v_i + g_i + l2_scale * l2_c * w32_i        (stored to v)
 *   d_i = lr * lr_factor_c * v_i
 *   n_c = sqrt(sum_i d_i^2),  s_c = max_change_c / n_c if max_change_c > 0 and n_c > max_change_c, else 1
 *   N   = sqrt(sum_c (s_c n_c)^2),  S = max_param_change / N if max_param_change > 0 and N > it, else 1
 *   w32_i -= S * s_c * d_i;  w16_i = rne_fp16(w32_i as stored)
 * A component is a set of segments [begin, end) of the buffer (elements); what no segment
 * covers is neither read nor written. Both tables live in device memory:
 *   segments  sorted by component (each component's segments are consecutive), disjoint,
 *             inside [0, n). A segment is cut into chunks of KF_UPD_CHUNK elements, one per
 *             workgroup; first_wg = the number of chunks of all segments before it,
 *             sum ceil((end - begin) / KF_UPD_CHUNK).
 *   comps     first_wg = the first_wg of the component's first segment, num_wg = the chunks
 *             of all its segments.
 * Segments may begin and end anywhere; the body of a chunk moves 16-byte vectors and needs
 * w32 / g / v 16-byte and w16 8-byte aligned bases. A table that breaks these rules gives
 * wrong sums but addresses nothing outside [0, n).
 * scratch: kf_update_scratch_bytes(n, nseg, ncomp) bytes of device memory, 8-byte aligned
 * (-1: bad arguments): fp32 [n / KF_UPD_CHUNK + nseg] per-workgroup sums of d^2 (one launch
 * slot per possible chunk), double [ncomp] (s_c n_c)^2, fp32 [ncomp] S * s_c * lr * lr_factor_c,
 * each rounded up to 256 bytes; written and read within the call.
 * stats: device fp32 [2 * ncomp + 2] = n_c [ncomp], s_c [ncomp], N, S of this call.
 * Three launches on the current stream: no host synchronisation, allocation or atomics;
 * every sum runs in a fixed order (the cross-workgroup ones in double), so the results are
 * bit-identical from run to run. */
#define KF_UPD_CHUNK 4096
typedef struct KfUpdSegment {
    long long begin, end;
    int comp, first_wg;
} KfUpdSegment;
typedef struct KfUpdComp {
    float max_change, l2, lr_factor; /* >= 0 (0: no limit), >= 0, > 0 */
    int first_wg, num_wg;
} KfUpdComp;
long long kf_update_scratch_bytes(long long n, int nseg, int ncomp);
int kf_update_maxchange(float *w32, void *w16, const float *g, float *v, long long n,
                        const KfUpdSegment *segments, int nseg, const KfUpdComp *comps, int ncomp,
                        float lr, float momentum, float max_param_change, float l2_scale,
                        void *scratch, float *stats);

/* ---- Dynamic loss scaling, kept on the device (csrc/loss_scale.hip) ----
 * The objective multiplies its derivative by `scale` before the one rounding to fp16
 * (kf_chain.h kf_chain_set_grad_scale); the backward is linear in the gradient, so the fp32
 * gradient buffer then holds scale * G. The update checks every trainable element of it for
 * a non-finite value, skips the step on one and unscales by 1 / scale otherwise. The rule is
 * kaldi_loss_scaler_update's (kaldi_bridge.h), per step, with `overflow` the check's answer:
 *   inv_used = 1 / scale                       (the scale this step's objective read)
 *   overflow:  skip = 1, scale = max(min_scale, scale * backoff), since = 0
 *   else:      skip = 0, ++since; since >= growth_interval: scale = min(max_scale, scale * growth), since = 0
 * The state is one block of device memory of kf_loss_scale_state_bytes() bytes, 16-byte
 * aligned, whose first float is the scale (the pointer kf_chain_set_grad_scale takes); the
 * options live in it. No host round trip, no atomics: the decision, the state and the skipped
 * step stay on the current stream.
 *   kf_loss_scale_init       state <- opts, scale = init_scale clamped to [min_scale, max_scale],
 *                            counters zero (one small launch); -1 on bad options
 *   kf_loss_scale_set_scale  scale <- value (clamped), since = 0 (a checkpoint restore, tests)
 *   kf_loss_scale_check      over the segments of a kf_update_maxchange table (comps are not read;
 *                            ncomp bounds a segment's comp), cut into the same KF_UPD_CHUNK chunks:
 *                            one flag per workgroup into scratch (kf_loss_scale_scratch_bytes(n, nseg)
 *                            bytes, 4-byte aligned), then one workgroup folds the flags and advances
 *                            the state by the rule above. What no segment covers is not read. Two launches.
 *   kf_loss_scale_read       synchronises the current stream; any pointer may be NULL
 *   kf_update_maxchange_scaled / kf_sgd_flat_scaled
 *                            the update calls with the state: every kernel loads skip and inv_used
 *                            block-uniformly, returns before it has written a byte on skip, and
 *                            uses g * inv_used otherwise. A skipped kf_update_maxchange_scaled
 *                            reports stats all zero (n_c = 0, s_c = 0, N = 0, S = 0: the norms are
 *                            not computed). state NULL: the plain call, launch for launch.
 * With a power of two as the scale g * inv_used is exact, and the update is bit-identical to
 * the plain one on the unscaled gradient. */
typedef struct KfLossScaleOpts {
    float init_scale, growth, backoff; /* 65536, 2, 0.5 */
    int growth_interval;               /* 2000 */
    float min_scale, max_scale;        /* 1, 65536 */
} KfLossScaleOpts;
void kf_loss_scale_default_opts(KfLossScaleOpts *opts);
long long kf_loss_scale_state_bytes(void);
long long kf_loss_scale_scratch_bytes(long long n, int nseg);
int kf_loss_scale_init(void *state, const KfLossScaleOpts *opts);
int kf_loss_scale_set_scale(void *state, float scale);
int kf_loss_scale_check(void *state, const float *g, long long n, const KfUpdSegment *segments, int nseg,
                        int ncomp, void *scratch);
int kf_loss_scale_read(const void *state, float *scale, int *since, long long *steps, long long *skipped,
                       int *last_overflow);
int kf_update_maxchange_scaled(float *w32, void *w16, const float *g, float *v, long long n,
                               const KfUpdSegment *segments, int nseg, const KfUpdComp *comps, int ncomp,
                               float lr, float momentum, float max_param_change, float l2_scale,
                               void *scratch, float *stats, const void *loss_scale_state);
int kf_sgd_flat_scaled(float *w32, void *w16, const float *g, float *v, float lr, float mom,
                       long long n, const void *loss_scale_state);

/* ---- Semi-orthogonal constraint (csrc/orthonormal.hip) ----
 * Kaldi's ConstrainOrthonormal over every constrained matrix of a flat parameter set in one
 * call. A matrix is W [K rows x n cols] (y = x W, the transpose of Kaldi's M: the columns
 * are constrained) at elements [offset, offset + K n) of w32 / w16, with a constraint value
 * c: 0 off, > 0 a fixed scale, < 0 the floating scale. On the fp32 weights:
 *   P = W^T W (fp32, exact f32-input MFMA),  nu = 0.125
 *   c < 0:  tP = tr P, tPP = sum P_ij^2 (double), s = sqrt(tPP / tP), ratio = tPP n / tP^2,
 *           nu *= 0.5 if ratio > 1.02, and again if ratio > 1.1
 *   c > 0:  s = c, ratio = 1
 *   Q = P - s^2 I,  err = sqrt(sum Q_ij^2)
 *   w32 -= 4 (nu / s^2) W Q;  w16 = rne_fp16(w32 as stored)
 * A matrix with tP == 0 or a non-finite s is left untouched and reports s = 0 (and ratio,
 * err, nu 0). Supported shapes: K % 32 == 0, n % 32 == 0, 32 <= n <= K, n <= 512; any other
 * shape with c != 0, a non-finite c or a matrix outside [0, n_params) returns -1 before
 * anything is launched. Matrices must not overlap; what no matrix covers is neither read nor
 * written, nor is a matrix with c == 0.
 * mats is the table in host memory (checked, sizes the launches), mats_dev the same table in
 * device memory (read by the kernels), uploaded once by the caller.
 * scratch: kf_orthonormal_scratch_bytes(mats, nmat) bytes of device memory, 16-byte aligned
 * (-1: a bad table): fp32 [nmat] factors 4 nu / s^2 rounded up to 256 bytes, then per
 * constrained matrix ceil(K / KF_ORTHO_KCHUNK) partial n x n tiles of P and the n x n Q;
 * written and read within the call.
 * stats: device fp32 [4 * nmat] = s, ratio, err, nu per matrix (zeros where c == 0).
 * Three launches on the current stream whatever nmat is (none when no c != 0): no host
 * synchronisation, allocation or atomics; every sum runs in a fixed order, so the results
 * are bit-identical from run to run. */
#define KF_ORTHO_KCHUNK 512
typedef struct KfOrthoMat {
    long long offset;
    int K, n;
    float c;
    int reserved; /* 0 */
} KfOrthoMat;
long long kf_orthonormal_scratch_bytes(const KfOrthoMat *mats, int nmat);
int kf_orthonormal_constrain(float *w32, void *w16, long long n_params, const KfOrthoMat *mats,
                             const KfOrthoMat *mats_dev, int nmat, void *scratch, float *stats);
/* ---- Natural-gradient preconditioning (csrc/natgrad.hip) ----
 * The online natural-gradient method of Povey, Zhang and Khudanpur (Kaldi's NG-SGD), batched
 * over a table of preconditioners. A preconditioner works on row vectors of dimension D with
 * rank R (8 <= R <= KF_NG_MAX_RANK, 2 R <= D); Rp = R rounded up to a multiple of 32. Its state:
 *   w32 [Rp x D] fp32 at elements [w_off, w_off + Rp D) of the fp32 state buffer; rows R .. Rp-1
 *       are zero (exact no-ops wherever W is used)
 *   w16 the same matrix in fp16, the copy the statistics GEMMs read, at elements
 *       [h_off, h_off + KF_NG_W16_HALFS(D, Rp)) of the fp16 state buffer: [Rp x ld] with
 *       ld = KF_NG_W16_LD(D) (rows padded with zeros to a multiple of 8), then column D - 1 once
 *       more as a contiguous [Rp] vector (the bias of H = X W^T when X ends in a column of ones)
 *   sc  doubles at [s_off, s_off + 2 + Rp): rho, t (the step count), d[Rp] (d_i = 0 for i >= R)
 * and its statistics of one minibatch X [N x D], fp32 at [st_off, st_off + KF_NG_STAT_FLOATS(D, Rp))
 * of the statistics buffer (H = X W^T):
 *   [0] trX = tr(X X^T), [1] N, [2 .. 31] unused
 *   L  [Rp x Rp] = H^T H           at KF_NG_STAT_L
 *   JT [D x Rp]  = X^T H = J^T     at KF_NG_STAT_JT(Rp)     (updating steps; K = J J^T is formed
 *                                                            from it in double by the state kernel)
 * With eta = min(0.9, 1 - exp(-N / num_samples_history)), beta = rho (1 + alpha) + alpha sum(d) / D,
 * e_i = 1 / (beta / d_i + 1), f_i = e_i^-1/2, dr_i = d_i + rho:
 *   gamma = sqrt(trX / (trX - sum_i (2 - e_i) L_ii))      (1 if either trace is 0 or not finite)
 *   Z  = (eta/N)^2 F K F + (eta/N)(1 - eta)(Dr F L F + F L F Dr) + (1 - eta)^2 Dr^2
 *   Z  = U diag(c) U^T, c descending; c_i = max(c_i, (rho (1 - eta))^2); s = sqrt(c)
 *   rho' = max(epsilon, ((eta/N) trX + (1 - eta)(D rho + sum(d)) - sum(s)) / (D - R))
 *   d'_i = max(s_i - rho', epsilon, delta max_j (s_j - rho'))
 *   W' = E'^1/2 diag(1/s) U^T ((eta/N) F J + (1 - eta) Dr F W),  E' from d', rho'
 * All of the state arithmetic runs in double; every sum has a fixed order, no atomics, no host
 * round trip and no allocation, so two runs give the same bits.
 * Tables: pres / comps in host memory (checked, size the launches) and the same tables in
 * device memory (read by the kernels), uploaded once by the caller. */
#define KF_NG_MAX_RANK 96
#define KF_NG_STAT_L 32
#define KF_NG_STAT_JT(Rp) (32 + (long long)(Rp) * (Rp))
#define KF_NG_STAT_FLOATS(D, Rp) (32 + (long long)(Rp) * (Rp) + (long long)(D) * (Rp))
#define KF_NG_W16_LD(D) (((D) + 7) / 8 * 8)
#define KF_NG_W16_HALFS(D, Rp) ((long long)(Rp) * (KF_NG_W16_LD(D) + 1))
#define KF_NG_REPORT 8 /* floats per preconditioner: gamma, rho, sum(d), t, flag, 0, 0, 0 */
typedef struct KfNgOpts {
    int rank_in, rank_out;     /* the network layer's ranks (kernels read the table's R): 20, 80 */
    int update_period;         /* 4 */
    float num_samples_history; /* 2000 */
    float alpha;               /* 4 */
    float epsilon, delta;      /* 1e-10, 5e-4 */
} KfNgOpts;
typedef struct KfNgPre {
    int D, R;
    long long w_off, h_off, s_off, st_off;
} KfNgPre;
/* a weight gradient G = [dW [K x N] at g + dw_off ; db [N] at g + db_off (db_off < 0: none)] with
 * the preconditioners of its two sides (an index into pres, or -1: that side is left as it is):
 * pres[pre_in].D == K + (db_off >= 0), pres[pre_out].D == N */
typedef struct KfNgComp {
    long long dw_off, db_off;
    int K, N, pre_in, pre_out;
} KfNgComp;
void kf_ng_default_opts(KfNgOpts *opts);
/* the default initial state: rho = d_i = epsilon, t = 0, R_0[i][j] = 1 / sqrt(ceil(D / R)) where
 * j % R == i (rows re-normalised to unit length), W_0 = E^1/2 R_0 */
int kf_ng_init(const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const KfNgOpts *opts, float *w32,
               void *w16, double *sc);
/* out[0] = sum of squares of the operand's elements (+ nrows with ones != 0: an appended column
 * of ones), summed over the source rows with their multiplicities under the operand's splice
 * (double, fixed order), rounded to fp32; out[1] = nrows: the head of a preconditioner's
 * statistics. fp16 operands with hout = 1, no mask and no time stride. */
int kf_ng_trx(const KfOperand *op, int ones, float *out);
/* gamma of every preconditioner from trX, diag L and the state; writes report[KF_NG_REPORT p ..]
 * = gamma, rho, sum(d), t, flag 0 */
int kf_ng_scales(const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const KfNgOpts *opts, const double *sc,
                 const float *stat, float *report);
/* G <- gamma_in gamma_out (G - W_in^T (W_in G)), then G <- G - (G W_out^T) W_out, in place on
 * every table entry, gamma from report (kf_ng_scales). Only the K N (+ N) elements of an entry
 * are read or written. scratch: kf_ng_apply_scratch_bytes (16-byte aligned device memory) */
long long kf_ng_apply_scratch_bytes(const KfNgComp *comps, int ncomp, const KfNgPre *pres, int npre);
int kf_ng_apply(float *g, long long n_grad, const KfNgComp *comps, const KfNgComp *comps_dev, int ncomp,
                const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const float *w32, const float *report,
                void *scratch);
/* one workgroup per preconditioner. update != 0: the state update above from L, JT, trX and N
 * (Z built and diagonalised by cyclic Jacobi sweeps in double in LDS), w32 / w16 / d / rho
 * replaced; a non-finite statistic, eigenvalue or result leaves them untouched and sets
 * report[KF_NG_REPORT p + 4] = 1. Either way t <- t + 1.
 * scratch: kf_ng_state_scratch_bytes (16-byte aligned device memory) */
long long kf_ng_state_scratch_bytes(const KfNgPre *pres, int npre);
int kf_ng_state(const KfNgPre *pres, const KfNgPre *pres_dev, int npre, const KfNgOpts *opts, int update,
                float *w32, void *w16, double *sc, const float *stat, void *scratch, float *report);

/* ---- Per-sequence dropout masks (csrc/dropout.hip) ----
 * Kaldi's GeneralDropoutComponent with continuous = true, time-period = 0, block-dim = dim: one
 * factor per (sequence b, column n), shared by every frame of the sequence and applied by the
 * fused GEMM epilogue (KfEpilogue.drop above):
 *   x = Philox4x32-10(counter = {step, ordinal, b, n / 4}, key = {seed low, seed high})[n % 4]
 *   u = (x >> 8) * 2^-24,  mask[b * ld + n] = fmaf(4 p, u, 1 - 2 p)        (fp32)
 * uniform on [1 - 2p, 1 + 2p) with mean 1. Stateless: the same (seed, step, ordinal) gives the
 * same mask, in one launch for all n layers (per KF_DROP_MAX of them); an entry with p = 0 is
 * skipped (nothing is written). 0 <= p <= 0.5, dim % 4 == 0, ld % 4 == 0, ld >= dim, 16-byte
 * aligned mask, 0 <= step < 2^32, B <= 65535. `layers` is a host array. */
#define KF_DROP_MAX 32
typedef struct KfDropLayer {
    float *mask;   /* device fp32 [B x ld] */
    long long ld;
    int dim;
    int ordinal;   /* the layer's place in the counter */
    float p;
    int reserved;  /* 0 */
} KfDropLayer;
int kf_dropout_masks(int n, const KfDropLayer *layers, int B, unsigned long long seed, long long step);
/* row_seg[r] = the sequence of GEMM row r (KfEpilogue.row_seg), from the device sequence offsets
 * dev_seq_off int[B + 1] (seq_off[0] = 0, seq_off[B] = T; B <= 1: one sequence, all zeros).
 * tc = 0: rows are the T frames. tc > 0: rows are the tc compact rows of the row-subsampled
 * step (the rule and its conditions as kf_gather_rows below). */
int kf_row_seg(int32_t *row_seg, const int *dev_seq_off, int B, int T, int tc0, int tc);

/* ---- SpecAugment masks of the spec-augment-layer (csrc/specaug.hip) ----
 * Kaldi's GeneralDropoutComponent with specaugment-max-proportion followed by its
 * SpecAugmentTimeMaskComponent. The rule:
 *
 * Layer keys: freq-max-proportion f in [0, 1] (default 0.5), time-zeroed-proportion z in
 * [0, 1) (default 0.2), time-mask-max-frames m >= 1 (default 10). D = the layer's dim,
 *   Z   = min(D, floor(D f + 0.5))                                     (max_bins)
 *   m_n = max(1, floor(m (1 - z) / z)), on the host in double, capped at 2^31 - 1, unused
 *         when z = 0                                                   (max_kept)
 * Random numbers: the Philox4x32-10 of csrc/dropout.hip,
 *   X(b, kind, i) = word i % 4 of Philox(counter {step, 0x80000000 | (2k + kind), b, i / 4},
 *                                        key = the seed's low and high words)
 * k the spec-augment layer's ordinal among spec-augment layers (the high bit keeps these
 * streams apart from dropout's, whose ordinals are non-negative ints),
 *   u24(x) = x >> 8,  randint(x, n) = (u24(x) n) >> 24, an integer in [0, n), exact in 64 bits.
 * Frequency band of sequence b (kind 0): count = randint(X(b,0,0), Z + 1),
 *   start = randint(X(b,0,1), D - count + 1); columns [start, start + count) are zeroed on
 *   every frame of the sequence: one band per sequence.
 * Time mask of sequence b (kind 1, only when z > 0): alternating regions tile the sequence's
 *   frames from its first frame. Region 0 is zeroed iff (float)u24(X(b,1,0)) 2^-24 < (float)z;
 *   region r is zeroed iff (region 0 is zeroed) XOR (r is odd);
 *   len_r = 1 + randint(X(b,1,1 + r), zeroed_r ? m : m_n); the last region is clipped at the
 *   sequence's end.
 * Output element (r, c) is the input's bit pattern when the row is kept and c lies outside the
 * band, else +0 (0x0000), also for a NaN, Inf or negative input: a select, not a multiply.
 * No rescaling. Test mode is the identity.
 *
 * kf_specaug_rows: one launch writes the mask of every frame: row_band[r] = -1 when the whole
 * row is zeroed, else start | count << 16, the band of the row's sequence (dim <= 32767).
 * dev_seq_off device int[B + 1] (seq_off[0] = 0, seq_off[B] = T); B <= 1 or NULL: one sequence
 * [0, T). One wavefront per sequence; no LDS, no atomics. 0 <= max_bins <= dim, 0 <= z < 1,
 * max_zeroed >= 1, max_kept >= 1, ordinal < 2^30, 0 <= step < 2^32.
 * kf_specaug_apply: the select on fp16 x [rows x dim] (leading dimension ldx) into y (ldy),
 * x == y allowed. 16 bytes per lane when dim, ldx and ldy are multiples of 8 and both pointers
 * are 16-byte aligned, else element by element; any dim in [1, 32767]. */
int kf_specaug_rows(int32_t *row_band, const int *dev_seq_off, int B, int T, int dim, int max_bins, float z,
                    int max_zeroed, int max_kept, unsigned ordinal, unsigned long long seed, long long step);
int kf_specaug_apply(const void *x, long long ldx, void *y, long long ldy, long long rows, int dim,
                     const int32_t *row_band);

/* ---- Training-mode BatchNorm of the TDNN-F layers (csrc/batchnorm.hip) ----
 * Kaldi's BatchNormComponent in training mode on r = rne_fp16(relu(affine + bias)), an fp16
 * [rows x D] tensor the affine GEMM wrote (no scale, shift, dropout or bypass in its epilogue).
 * Every fp16 tensor: 16-byte aligned, ld >= D, ld % 8 == 0; D % 8 == 0; the per-column fp32
 * arrays of the apply entries 16-byte aligned. Column sums are taken in double, in a fixed order,
 * without atomics (two launches: per chunk of 256 rows, then over the chunks), so every entry
 * replays bit for bit. The partials live in the current stream's scratch.
 *
 * kf_bn_train_stats, per column c over the n = rows rows:
 *   mean = sum r / n,  var = max(0, sum r^2 / n - mean^2),
 *   scale = target_rms (var + eps)^-1/2,  shift = -mean scale
 * in double, stored in fp32. With the accumulators (device doubles: count [1], sum [D],
 * sumsq [D]; all three or none): count += n, sum += sum r, sumsq += sum r^2.
 * kf_bn_train_apply: out = rne_fp16(((r scale + shift) drop[row_seg[row]]) + alpha resid), the
 *   fp32 operations of the fused epilogue in its order (fmaf, multiply, fmaf); drop (fp32
 *   [B x ld_drop], ld_drop % 4 == 0, with row_seg) and resid (fp16, ldr) are optional.
 * kf_bn_train_bwd_stats: with g the gradient at the layer's output, dy = g drop[row_seg[row]] and
 *   yhat = (r scale + shift) / target_rms:  a = sum dy / n,  b = sum dy yhat / n  (fp32 stores of
 *   double sums; sum dy yhat = (scale sum dy r + shift sum dy) / target_rms).
 * kf_bn_train_bwd_apply: dz = rne_fp16(scale (dy - a - yhat b) relu_bit), the exact derivative
 *   through the batch statistics (eps included: scale carries it), Kaldi's
 *   BatchNormComponent::Backprop; evaluated in double. relu_bit is bit (row ld_mask + c) of the
 *   forward's ReLU mask (ld_mask in bits, a multiple of 8); mask == NULL: a BatchNorm with no ReLU
 *   below it, relu_bit = 1 (ld_mask ignored). dz may not alias g or r.
 * kf_bn_train_bwd_stats_rows / kf_bn_train_bwd_apply_rows: the backward of
 *   kf_bn_train_stats over the first stat_rows rows followed by kf_bn_train_apply over all `rows`
 *   (1 <= stat_rows <= rows, else -1). The sums run over every row, the divisor is n = stat_rows:
 *   a = sum_{row < rows} dy / n, b = sum_{row < rows} dy yhat / n; then
 *   dz = rne_fp16(scale (dy - a - yhat b) relu_bit) for row < stat_rows and
 *   dz = rne_fp16(scale dy relu_bit) from there on (those rows' r is not in the statistics). Same
 *   shape rules, sums and order; stat_rows == rows is kf_bn_train_bwd_stats / _apply bit for bit.
 *
 * Block statistics: a BatchNorm with block-dim = F on r [rows x H F], where column
 * h F + f belongs to block f (a conv layer: H = height-out, F = num-filters-out) and every sum runs
 * over the n = rows H block rows. F % 8 == 0, H >= 1, ld >= H F, ld % 8 == 0, rows <= 65535 x 64;
 * outputs and accumulators are [F] (count [1], += n). The rule, the double sums in a fixed order
 * and the two launches are kf_bn_train_stats' / kf_bn_train_bwd_stats' (no dropout table); the lane
 * map is made for the tall, narrow case: a lane keeps 8 columns of one block for its whole walk,
 * the lanes of a workgroup share 64 tensor rows, a second launch adds the workgroups' partials
 * with 32 lanes per column. The apply entries above serve a dense r through its [rows H x F],
 * ld = F view. */
int kf_bn_train_stats(const void *r, long long ld, int rows, int D, float eps, float target_rms, float *mean,
                      float *var, float *scale, float *shift, double *acc_count, double *acc_sum, double *acc_sumsq);
int kf_bn_train_apply(const void *r, long long ld, int rows, int D, const float *scale, const float *shift,
                      const float *drop, long long ld_drop, const int32_t *row_seg, const void *resid, long long ldr,
                      float alpha, void *out, long long ldo);
int kf_bn_train_bwd_stats(const void *g, long long ldg, const void *r, long long ldr, int rows, int D,
                          const float *scale, const float *shift, float target_rms, const float *drop,
                          long long ld_drop, const int32_t *row_seg, float *a, float *b);
int kf_bn_train_bwd_apply(const void *g, long long ldg, const void *r, long long ldr, int rows, int D,
                          const float *scale, const float *shift, float target_rms, const float *a, const float *b,
                          const float *drop, long long ld_drop, const int32_t *row_seg, const uint8_t *mask,
                          long long ld_mask, void *dz, long long lddz);
int kf_bn_train_bwd_stats_rows(const void *g, long long ldg, const void *r, long long ldr, int rows, int stat_rows, int D,
                               const float *scale, const float *shift, float target_rms, const float *drop,
                               long long ld_drop, const int32_t *row_seg, float *a, float *b);
int kf_bn_train_bwd_apply_rows(const void *g, long long ldg, const void *r, long long ldr, int rows, int stat_rows, int D,
                               const float *scale, const float *shift, float target_rms, const float *a, const float *b,
                               const float *drop, long long ld_drop, const int32_t *row_seg, const uint8_t *mask,
                               long long ld_mask, void *dz, long long lddz);
int kf_bn_block_stats(const void *r, long long ld, int rows, int H, int F, float eps, float target_rms, float *mean,
                      float *var, float *scale, float *shift, double *acc_count, double *acc_sum, double *acc_sumsq);
int kf_bn_block_bwd_stats(const void *g, long long ldg, const void *r, long long ldr, int rows, int H, int F,
                          const float *scale, const float *shift, float target_rms, float *a, float *b);

/* ---- ReLU unit statistics and self-repair (csrc/batchnorm.hip) ----
 * Kaldi's StoreStats and RectifiedLinearComponent::RepairGradients for a ReLU whose output r the
 * training-mode BatchNorm entries above read. Same alignment and shape rules as those entries.
 *
 * kf_bn_train_stats_relu / kf_bn_block_stats_relu: kf_bn_train_stats / kf_bn_block_stats, and from
 *   the same pass over r: relu_count[0] += n, relu_deriv[c] += #{rows : r > 0} (device doubles
 *   [1], [D] or [F]; the counts are integers, exact; fixed order, no atomics). Both NULL: the
 *   launches and every output bit of the plain entry; one of them NULL: -1.
 * kf_relu_repair_vectors: one launch for the n sites of a table (given on the host, for the
 *   checks, and on the device). Per site and column, in double:
 *     count == 0                 : s = 0
 *     deriv <= lower count       : s = -scale S   (a dead unit)
 *     deriv >  upper count       : s = +scale S   (a saturated unit)
 *     otherwise                  : s = 0
 *   S = *loss_scale_dev (a device float), 1 when NULL; scale S is one fp32 product. s is fp32 [D],
 *   16-byte aligned; D % 8 == 0, scale >= 0, 0 <= lower < upper <= 1.
 * kf_bn_train_bwd_apply_repair / kf_bn_train_bwd_apply_rows_repair: the two apply entries with
 *   dz = rne_fp16(scale (dy - a - yhat b) relu_bit + repair[c]), the term inside the one rounding
 *   (so an element whose relu_bit is 0 stores rne_fp16(repair[c])); in the _rows form on the rows
 *   < stat_rows only, the rows from there on are the plain entry's. repair is fp32 [D], 16-byte
 *   aligned; NULL is the plain entry. Two launches: the plain entry's kernel, then one that
 *   evaluates the columns with repair[c] != 0 again on the statistics rows; every other element
 *   keeps the plain kernel's bits, so an all-zero repair is the plain entry bit for bit. The second
 *   launch reads g and r again: dz equal to g or r returns -1. */
typedef struct {
    const double *count; /* [1] */
    const double *deriv; /* [D] */
    float *s;            /* [D] out */
    int D;
    float scale;
    double lower, upper;
} KfRepairSite;
int kf_bn_train_stats_relu(const void *r, long long ld, int rows, int D, float eps, float target_rms, float *mean,
                           float *var, float *scale, float *shift, double *acc_count, double *acc_sum, double *acc_sumsq,
                           double *relu_count, double *relu_deriv);
int kf_bn_block_stats_relu(const void *r, long long ld, int rows, int H, int F, float eps, float target_rms, float *mean,
                           float *var, float *scale, float *shift, double *acc_count, double *acc_sum, double *acc_sumsq,
                           double *relu_count, double *relu_deriv);
int kf_relu_repair_vectors(const KfRepairSite *sites, const KfRepairSite *sites_dev, int n, const float *loss_scale_dev);
int kf_bn_train_bwd_apply_repair(const void *g, long long ldg, const void *r, long long ldr, int rows, int D,
                                 const float *scale, const float *shift, float target_rms, const float *a, const float *b,
                                 const float *drop, long long ld_drop, const int32_t *row_seg, const uint8_t *mask,
                                 long long ld_mask, void *dz, long long lddz, const float *repair);
int kf_bn_train_bwd_apply_rows_repair(const void *g, long long ldg, const void *r, long long ldr, int rows, int stat_rows,
                                      int D, const float *scale, const float *shift, float target_rms, const float *a,
                                      const float *b, const float *drop, long long ld_drop, const int32_t *row_seg,
                                      const uint8_t *mask, long long ld_mask, void *dz, long long lddz, const float *repair);

/* row sets of the row-subsampled train step (kf_nnet.h nnet_set_row_subsampling): compact
 * row c is source row 3c for c < tc0, else (T-1) - 3(tc-1-c). row_bytes % 16 == 0.
 * Every source row must exist: 3(tc0-1) <= T-1 and, with a tail (tc > tc0), its lowest row
 * (T-1) - 3(tc-tc0-1) >= 0 (tail rows may lie between head rows); anything else returns -1.
 * gather: dst[c] = src[row(c)] for c < tc; scatter: every full row t < T of dst gets the
 * compact row of src whose source row is t, or zeros */
int kf_gather_rows(void *dst, const void *src, long long row_bytes, int T, int tc0, int tc);
int kf_scatter_rows(void *dst, const void *src, long long row_bytes, int T, int tc0, int tc);
/* kf_scatter_rows for the full rows r0 .. T-1 only, dst row 0 = full row r0 */
int kf_scatter_rows_from(void *dst, const void *src, long long row_bytes, int T, int tc0, int tc, int r0);
/* edge[c] = rne(sum over rows[0..n) in that order of src[rows[i] * ld + c]), n <= 4 (host array) */
int kf_rows_sum_list(void *edge, const void *src, long long ld, const int *rows, int n, int cols);
const char *kf_layers_last_error(void);

/* Kaldi compressed-matrix expansion (egs input, kf_egs.h). One descriptor per stored
 * matrix; payload_off = byte offset of its payload in the device blob (2-byte aligned,
 * 4 for FM); rows land at out rows [out_row, out_row + rows). cols <= 256. */
enum { KF_CM_ONEBYTE_COLHDR = 1, KF_CM_TWOBYTE = 2, KF_CM_ONEBYTE = 3, KF_CM_FLOAT = 4 };
typedef struct {
    int format, rows, cols, out_row;
    float min_value, range;
    long long payload_off;
} KfCmDesc;
int kf_cm_expand(const KfCmDesc *dev_desc, int nmat, int max_rows, int max_cols,
                 const void *dev_blob, void *dev_out, int ldo);
/* Same from host arrays: every descriptor is bounds-checked against blob_bytes, then
 * descriptors + blob travel in one pinned, stream-ordered H2D copy (kf_get_stream())
 * ahead of the launch. The host arrays may be freed on return. */
int kf_cm_expand_host(const KfCmDesc *desc, int nmat, int max_rows, int max_cols,
                      const void *blob, size_t blob_bytes, void *dev_out, int ldo);

/* Restricted self-attention of attention-relu-batchnorm layers (csrc/attention.hip;
 * forward.go:795-909 runs it on the CPU). proj: fp16 [T x ldp] affine output, per head
 * [key kd | value vd | query key kd | query context ctx]; frame t attends to rows
 * t + (o - num_left) * stride, o < context, zero outside [0, T). */
typedef struct {
    const void *proj;
    long long ldp;
    int T, num_heads, key_dim, value_dim, context, num_left, stride;
    float key_scale;
} KfAttention;
/* out: fp16 [T x ldo], width num_heads * (value_dim + context); y = bn(relu(att));
 * mask (may be NULL): ReLU bits, row-major over width (width % 8 == 0). */
int kf_attention_forward(const KfAttention *a, void *out, long long ldo, uint8_t *mask, const float *scale,
                         const float *shift);
/* dz: fp16 gradient at the attention output (pre-ReLU) [T x ldz]; dproj: fp16, same
 * layout and ld as proj (every element written); scratch: fp32 [2 x T x heads x context]. */
int kf_attention_backward(const KfAttention *a, const void *dz, long long ldz, void *dproj, float *scratch);

/* ivector input path (csrc/ivector.hip). dev_seq_off: device int[B+1] frame offsets of
 * the sequences (seq_off[B] = T); NULL in kf_combine_feature_maps = b is frame-level.
 * combine: out[t][h*(nf1+nf2) + f] = f < nf1 ? a[t][h*nf1 + f] : b[seq(t)][h*nf2 + f-nf1] */
int kf_combine_feature_maps(const void *a, long long lda, const void *b, long long ldb, const int *dev_seq_off,
                            int B, void *out, long long ldo, int T, int height, int nf1, int nf2);
/* db[s][h*nf2 + g] = sum over the frames t of sequence s of dy[t][h*(nf1+nf2) + nf1 + g] */
int kf_combine_feature_maps_backward(const void *dy, long long ldy, const int *dev_seq_off, int B, void *db,
                                     long long ldb, int height, int nf1, int nf2);
/* small num-filters-in convolution as im2col + GEMM: P [T*hout x kp], column tap*fin + c
 * = x[t + dt[tap]][ho*sub + dh[tap]][c] (zero outside), columns >= ntaps*fin zero */
int kf_im2col_small(const void *x, long long ldx, int T, int hin, int hout, int sub, int fin, int ntaps,
                    const int *dt, const int *dh, void *P, int kp);
/* its transpose, gather form: dx [T x hin*fin] */
int kf_col2im_small(const void *dP, int T, int hin, int hout, int sub, int fin, int ntaps, const int *dt,
                    const int *dh, int kp, void *dx, long long ldx);
/* per-sequence linear-component on R rows, any dims: y = x . W (fp32 accumulation) and
 * its weight gradient dW = x^T . g (fp32, overwritten, summed in row order) */
int kf_rows_gemm(const void *x, long long ldx, const void *W, long long ldw, void *y, long long ldy, int R, int K,
                 int N);
int kf_rows_wgrad(const void *x, long long ldx, const void *g, long long ldg, float *dW, long long ldd, int R, int M,
                  int N);
/* y[r][c] = rne_fp16(fp32(x[r][c] * scale[c])) (fp16 in / out, fp32 scale; x may be y) */
int kf_scale_cols(const void *x, long long ldx, const float *scale, void *y, long long ldy, int rows, int cols);

/* optional HIP-event timing of the step's kernel classes on the stream each runs on;
 * collect sums since reset. Classes: 0 = kf_gemm_fused on the tiled GEMM, 1 = kf_gemm_wgrad
 * GEMM, 2 = chain numerator (flops = arc updates), 3 = chain den (flops = algorithmic
 * L2/HBM bytes), 4 = kf_gemm_fused on the 3x3 conv halo kernel, 5 = the conv halo weight
 * gradient, 6 = the split-K slab reduce (bytes only) */
void kf_prof_enable(int on);
/* pre-create the timing events of n profiled launches (no event creation in timed code) */
int kf_prof_reserve(int n);
int kf_prof_collect(int cls, long long *count, double *ms, double *flops);
/* the same plus the algorithmic HBM bytes of those launches (GEMM classes: each
 * operand's source tensor read once, epilogue tensors read / written once) */
int kf_prof_collect2(int cls, long long *count, double *ms, double *flops, double *bytes);
void kf_prof_reset(void);

/* test hook: the fused GEMM's K-step interleave of a two-part spliced A with parts of
 * >= 512 columns (the TDNN-F linear forward / affine input gradient). 1 (default):
 * the K-steps alternate between the parts; 0: part order. Only the fp32 accumulation
 * order differs. */
void kf_gemm_debug_kil(int on);
/* test hook: 1 (default): the long-K N = 160 / 320 products on a two-part spliced A (parts of
 * >= 512 columns, |dt| <= 8, no mask / MXFP8 / dropout / out8) whose 128x160 tiles number at
 * most 256 go to the single-staging kernel (source rows in LDS once per 64-column chunk,
 * both parts read from that image); 0: to the tiled kernel; 2: to the single-staging kernel at
 * every row count (measurements). The outputs are bit-identical. */
void kf_gemm_debug_splice_once(int on);
/* diagnostics (tests): the single-staging kernel's plan. out[0] = 1, out[1] = 1 when the kernel
 * applies (kf_splice_once_debug_last: was launched), else 0 and the rest zero; out[2..] = BM, BN,
 * the parts' row span max(dt) - min(dt), edge-row slots, zero slots, image rows (= BM + span +
 * edge slots + zero slots), 1 KiB pieces per image, images in the ring, B ring stages, dynamic
 * LDS bytes, row tiles, column tiles, B k-contiguous. Writes min(n, 16) ints, returns that count.
 * _plan: for the given product, without a launch or any HIP call (-1: an invalid operand);
 * _last: of the calling thread's last kf_gemm_fused that reached this dispatch. */
int kf_splice_once_debug_plan(int M, int N, int K, const KfOperand *A, const KfOperand *B,
                              const KfEpilogue *epi, int *out, int n);
int kf_splice_once_debug_last(int *out, int n);
/* n <= KF_TRANSPOSE_MAX fp16 transposes in one launch: dst[j] [N[j] x M[j]] = src[j]^T
 * (src[j] [M[j] x N[j]] row-major); the network's transposed weight copies */
#define KF_TRANSPOSE_MAX 48
int kf_transpose_batch(int n, const void *const *src, void *const *dst, const int *M, const int *N);
/* diagnostics: wall-clock stamps (100 MHz) of block 300, wave 0 of the conv-halo launch
 * number `at` counted from this call: [0] start, [1 + 2s] after step s's wait and barrier,
 * [2 + 2s] after its MFMAs, [126] before the epilogue, [127] end; buf NULL disarms */
void kf_halo_trace(unsigned long long *buf, int at);
/* diagnostics (tests): what the calling thread's last halo dispatch chose, read-only (no
 * launch depends on it). out[0] = 0 none yet, 1 the last kf_gemm_fused that reached the conv
 * halo dispatch, 2 the last kf_gemm_wgrad that reached the halo weight gradient's; out[1] = 1
 * when the halo kernel was launched, 0 when the dispatch declined (the rest is then zero).
 *   kind 1: out[2..] = BM, BN, BROW (B as shifted weight rows), nch (64-channel chunks),
 *           nbuf (halo images), hpe, hpos (halo row pitch), pitch pad taken, row tiles,
 *           column tiles
 *   kind 2: out[2..] = BN, waves, stages, npieces, hpw, splits, kps
 * Writes min(n, 16) ints (unused ones zero) and returns that count. */
int kf_halo_debug_last(int *out, int n);
/* diagnostics: phase stamps of block `blk` and {start, end, hw id | xcc << 32} of every
 * block of gemm_kernel launch number `at` (counted from this call), wall_clock64 ticks
 * (100 MHz); buf holds 64 + 3 * blocks words; null = off */
void kf_gemm_trace(unsigned long long *buf, int at, int blk);

const char *kf_last_error(void);
void kf_clear_error(void);
/* diagnostics: the kf_prof records since the last kf_prof_reset in issue order (class,
 * milliseconds, flops, and per record 4 ints: M, N, K, BM * 10000 + BN; zeros for
 * brackets that are not one GEMM launch); returns the count written (at most max) */
int kf_prof_records(int max, int *cls, float *ms, double *flops, int *mnkt);

/* Error hygiene across the C-ABI. HIP keeps one pending error per host
 * thread, read and reset by hipGetLastError(). Every entry point of this library that
 * checks its own launches with hipGetLastError() first calls kf_take_pending(its name):
 * an error some earlier HIP call left pending (another library, the caller's own HIP
 * calls, or a runtime call whose status nobody read) is consumed there and logged as
 * "pending before <where>: <error>" instead of being reported as that entry's failure.
 * kf_take_pending returns the consumed hipError_t (0 = none). kf_pending_log returns
 * the log since the last kf_pending_clear (NULL if empty; at most the last 16 notes,
 * plus the total count); kf_peek_error returns the pending error without consuming
 * it. With KF_ERR_VERBOSE=1 in the environment every note is also printed to stderr. */
int kf_take_pending(const char *where);
const char *kf_pending_log(void);
void kf_pending_clear(void);
int kf_peek_error(void);
/* diagnostics (tests): one workgroup spinning for `cycles` GPU clock cycles on `stream` */
int kf_debug_spin(void *stream, long long cycles);

#ifdef __cplusplus
}
#endif
#endif
