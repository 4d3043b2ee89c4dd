// batchnorm.hip — training-mode BatchNorm (kf_ops.h kf_bn_train_*, kf_bn_block_*; DESIGN.md §23,
// §27): Kaldi's BatchNormComponent in training mode. The affine GEMM writes
// r = rne_fp16(relu(affine + bias)) and its ReLU mask; the four kf_bn_train_* entries normalise r
// by the minibatch's own column statistics and differentiate through them. The kf_bn_block_*
// entries further down take the statistics of a BatchNorm with a block dimension (a conv layer).
//
// Column sums are taken in double, in a fixed order and without atomics, so a step replays bit
// for bit: a first launch reduces each chunk of kChunk rows to one partial per column (a lane
// walks its rows in order, the 4 row lanes of a workgroup are summed in order through LDS), a
// second sums the chunks in a fixed order (eight interleaved runs per column, added in order
// through LDS) and finishes. All four entries are bound by HBM: every input is read once with
// 16-byte lanes along the row, every output written once.
#include "kf_common.h"
#include "../../include/kf_ops.h"

namespace {

constexpr int kThreads = 256;
constexpr int kColLanes = 64;               // lanes along a row, 8 halves (16 bytes) each: a wave reads 1 KB
constexpr int kRowLanes = kThreads / kColLanes;
constexpr int kSlab = kColLanes * 8;        // columns of a workgroup
// rows of a chunk: 96,000 x 1536 (the benchmark model's TDNN-F output) gives 375 x 3 = 1125
// workgroups of 256 threads, more than four per CU of the MI355X's 256
constexpr int kChunk = 256;
// the second launch: a workgroup finishes kFinCols columns, kFinLanes lanes per column; lane l sums
// the chunks l, l + kFinLanes, ... in order, then the lanes are added in order
constexpr int kFinCols = 32;
constexpr int kFinLanes = kThreads / kFinCols;

struct Drop {
    const float *tab;  // [B x ld] or null
    long long ld;
    const int32_t *row_seg;
};

__device__ __forceinline__ void load_f8(const float *p, float (&v)[8]) {
    const float4v lo = *reinterpret_cast<const float4v *>(p), hi = *reinterpret_cast<const float4v *>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = lo[e];
        v[e + 4] = hi[e];
    }
}

// the row lanes' sums of a column, added in lane order; part[(2 chunk + k) * D + col]
__device__ __forceinline__ void reduce_store(double (&s0)[8], double (&s1)[8], double *part, int D) {
    __shared__ double red[kRowLanes][kSlab];
    const int cx = threadIdx.x % kColLanes, ry = threadIdx.x / kColLanes;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[ry][cx * 8 + e] = k ? s1[e] : s0[e];
        __syncthreads();
        for (int cl = threadIdx.x; cl < kSlab && blockIdx.x * kSlab + cl < D; cl += kThreads) {
            double t = red[0][cl];
#pragma unroll
            for (int y = 1; y < kRowLanes; ++y) t += red[y][cl];
            part[((long long)blockIdx.y * 2 + k) * D + blockIdx.x * kSlab + cl] = t;
        }
        __syncthreads();
    }
}

// the row lanes' counts of a column (kf_bn_train_stats_relu), added in lane order;
// cnt[chunk * D + col]. Integers: exact in any order, and the order is fixed all the same.
__device__ __forceinline__ void reduce_store_count(const int (&n)[8], unsigned *cnt, int D) {
    __shared__ int redn[kRowLanes][kSlab];
    const int cx = threadIdx.x % kColLanes, ry = threadIdx.x / kColLanes;
#pragma unroll
    for (int e = 0; e < 8; ++e) redn[ry][cx * 8 + e] = n[e];
    __syncthreads();
    for (int cl = threadIdx.x; cl < kSlab && blockIdx.x * kSlab + cl < D; cl += kThreads) {
        int t = redn[0][cl];
#pragma unroll
        for (int y = 1; y < kRowLanes; ++y) t += redn[y][cl];
        cnt[(long long)blockIdx.y * D + blockIdx.x * kSlab + cl] = (unsigned)t;
    }
}

// partials of sum r and sum r^2 (one conversion to double per element; its square is exact there)
// COUNT (k_bn_fwd_part_relu only): also the number of elements r > 0, from the same registers.
// COUNT false is the code the kernel always was, under the symbol it always had.
template <bool COUNT>
__device__ __forceinline__ void bn_fwd_part_body(const h16 *r, long long ld, int rows, int D, double *part, unsigned *cnt) {
    const int cx = threadIdx.x % kColLanes, ry = threadIdx.x / kColLanes;
    const int c0 = blockIdx.x * kSlab + cx * 8;
    const int r0 = blockIdx.y * kChunk, r1 = min(rows, r0 + kChunk);
    double s0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c0 < D) {
#pragma unroll 4
        for (int m = r0 + ry; m < r1; m += kRowLanes) {
            const half8 v = load_h8(r + (long long)m * ld + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double x = (double)h2f(v[e]);
                s0[e] += x;
                s1[e] = fma(x, x, s1[e]);
                if constexpr (COUNT) n[e] += x > 0.0 ? 1 : 0;
            }
        }
    }
    reduce_store(s0, s1, part, D);
    if constexpr (COUNT) reduce_store_count(n, cnt, D);
}
__global__ __launch_bounds__(kThreads) void k_bn_fwd_part(const h16 *r, long long ld, int rows, int D, double *part) {
    bn_fwd_part_body<false>(r, ld, rows, D, part, nullptr);
}
__global__ __launch_bounds__(kThreads) void k_bn_fwd_part_relu(const h16 *r, long long ld, int rows, int D, double *part,
                                                                unsigned *cnt) {
    bn_fwd_part_body<true>(r, ld, rows, D, part, cnt);
}

// partials of sum dy and sum dy r, dy = g * drop[row_seg[row]] (exact in double)
template <bool DROP>
__global__ __launch_bounds__(kThreads) void k_bn_bwd_part(const h16 *g, long long ldg, const h16 *r, long long ldr,
                                                          int rows, int D, Drop dr, double *part) {
    const int cx = threadIdx.x % kColLanes, ry = threadIdx.x / kColLanes;
    const int c0 = blockIdx.x * kSlab + cx * 8;
    const int r0 = blockIdx.y * kChunk, r1 = min(rows, r0 + kChunk);
    double s0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c0 < D) {
#pragma unroll 2
        for (int m = r0 + ry; m < r1; m += kRowLanes) {
            const half8 gv = load_h8(g + (long long)m * ldg + c0);
            const half8 rv = load_h8(r + (long long)m * ldr + c0);
            float d[8];
            if constexpr (DROP) load_f8(dr.tab + (long long)dr.row_seg[m] * dr.ld + c0, d);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                double dy = (double)h2f(gv[e]);
                if constexpr (DROP) dy *= (double)d[e];
                s0[e] += dy;
                s1[e] = fma(dy, (double)h2f(rv[e]), s1[e]);
            }
        }
    }
    reduce_store(s0, s1, part, D);
}

// sum and sum of squares of column c over the chunks, in the fixed order above; valid in lane 0.
// COLS columns of a workgroup, kThreads / COLS lanes per column (kFinCols for the column entries,
// kBlkFinCols for the block entries below)
template <int COLS>
__device__ __forceinline__ void sum_chunks(const double *part, int nchunk, int D, int c, int lane, double &s, double &q) {
    constexpr int LANES = kThreads / COLS;
    __shared__ double red[2][LANES][COLS];
    double s0 = 0.0, q0 = 0.0;
    if (c < D) {
#pragma unroll 4
        for (int k = lane; k < nchunk; k += LANES) {
            s0 += part[((long long)k * 2) * D + c];
            q0 += part[((long long)k * 2 + 1) * D + c];
        }
    }
    red[0][lane][threadIdx.x % COLS] = s0;
    red[1][lane][threadIdx.x % COLS] = q0;
    __syncthreads();
    s = red[0][0][threadIdx.x % COLS];
    q = red[1][0][threadIdx.x % COLS];
    if (lane == 0) {
#pragma unroll
        for (int l = 1; l < LANES; ++l) {
            s += red[0][l][threadIdx.x % COLS];
            q += red[1][l][threadIdx.x % COLS];
        }
    }
}

// forward: the chunks in order, then mean, var (floored at 0), scale = rms (var + eps)^-1/2 and
// shift = -mean scale in double, stored in fp32; the accumulators take the sums as they are
// COUNT (k_bn_fwd_finish_relu only): the chunks' counts of r > 0 in the same order, into
// the ReLU statistics relu_count += rows, relu_deriv[c] += count (doubles holding integers: exact)
template <int COLS, bool COUNT>
__device__ __forceinline__ void bn_fwd_finish_body(const double *part, int nchunk, double rows, int D, double eps, double rms,
                                                   float *mean, float *var, float *scale, float *shift, double *acc_count,
                                                   double *acc_sum, double *acc_sumsq, const unsigned *cnt,
                                                   double *relu_count, double *relu_deriv) {
    const int c = blockIdx.x * COLS + threadIdx.x % COLS, lane = threadIdx.x / COLS;
    double s, q;
    sum_chunks<COLS>(part, nchunk, D, c, lane, s, q);
    if constexpr (COUNT) {
        constexpr int LANES = kThreads / COLS;
        __shared__ unsigned long long redn[LANES][COLS];
        unsigned long long n0 = 0;
        if (c < D)
            for (int k = lane; k < nchunk; k += LANES) n0 += cnt[(long long)k * D + c];
        redn[lane][threadIdx.x % COLS] = n0;
        __syncthreads();
        if (c < D && lane == 0) {
            unsigned long long n = redn[0][threadIdx.x % COLS];
#pragma unroll
            for (int l = 1; l < LANES; ++l) n += redn[l][threadIdx.x % COLS];
            relu_deriv[c] += (double)n;
            if (c == 0) relu_count[0] += rows;
        }
    }
    if (c >= D || lane != 0) return;
    const double mu = s / rows;
    double v = q / rows - mu * mu;
    v = v > 0.0 ? v : 0.0;
    const double sc = rms / sqrt(v + eps);
    mean[c] = (float)mu;
    var[c] = (float)v;
    scale[c] = (float)sc;
    shift[c] = (float)(-mu * sc);
    if (acc_sum) {
        acc_sum[c] += s;
        acc_sumsq[c] += q;
        if (c == 0) acc_count[0] += rows;
    }
}
template <int COLS>
__global__ __launch_bounds__(kThreads) void k_bn_fwd_finish(const double *part, int nchunk, double rows, int D, double eps,
                                                            double rms, float *mean, float *var, float *scale,
                                                            float *shift, double *acc_count, double *acc_sum,
                                                            double *acc_sumsq) {
    bn_fwd_finish_body<COLS, false>(part, nchunk, rows, D, eps, rms, mean, var, scale, shift, acc_count, acc_sum, acc_sumsq,
                                    nullptr, nullptr, nullptr);
}
template <int COLS>
__global__ __launch_bounds__(kThreads) void k_bn_fwd_finish_relu(const double *part, int nchunk, double rows, int D, double eps,
                                                                 double rms, float *mean, float *var, float *scale,
                                                                 float *shift, double *acc_count, double *acc_sum,
                                                                 double *acc_sumsq, const unsigned *cnt, double *relu_count,
                                                                 double *relu_deriv) {
    bn_fwd_finish_body<COLS, true>(part, nchunk, rows, D, eps, rms, mean, var, scale, shift, acc_count, acc_sum, acc_sumsq, cnt,
                                   relu_count, relu_deriv);
}

// backward: a = sum dy / n, b = sum dy yhat / n with yhat = (r scale + shift) / rms, so
// sum dy yhat = (scale sum dy r + shift sum dy) / rms
template <int COLS>
__global__ __launch_bounds__(kThreads) void k_bn_bwd_finish(const double *part, int nchunk, double rows, int D,
                                                            const float *scale, const float *shift, double inv_rms,
                                                            float *a, float *b) {
    const int c = blockIdx.x * COLS + threadIdx.x % COLS, lane = threadIdx.x / COLS;
    double s, q;
    sum_chunks<COLS>(part, nchunk, D, c, lane, s, q);
    if (c >= D || lane != 0) return;
    a[c] = (float)(s / rows);
    b[c] = (float)(((double)scale[c] * q + (double)shift[c] * s) * inv_rms / rows);
}

// ---- block statistics (kf_bn_block_*): r [rows x H F], column h F + f belongs to
// block f, the sums run over the n = rows H block rows (row, h) of F columns each. Built for the
// tall, narrow case (a conv layer: 3.84 M block rows of 64 columns), where the column kernels
// above would leave seven of eight column lanes idle.
//
// Lane map. The F columns are cw = min(F / 8, kThreads) groups of 8 (a slab of kThreads groups
// per blockIdx.x when F > 8 kThreads); thread t keeps group t % cw for its whole walk and is
// position p = t / cw of P = kThreads / cw. Position p walks the workgroup's block rows p, p + P,
// ... in order, so its 2 x 8 double accumulators never change meaning, and consecutive lanes read
// consecutive 16 bytes: with F = 64 a wave reads 8 whole block rows, 1 KB in one piece when
// ld = H F. (row, h) advance by (P / H, P % H) with one carry: no division in the loop.
constexpr int kBlkRows = 64;  // tensor rows of a workgroup: 96,000 rows give 1500 workgroups, 5.9 per CU
// the second launch: a workgroup finishes kBlkFinCols columns (one 64-byte line of partials),
// 32 lanes per column: 1500 partials are 47 dependent steps of a lane, not 188
constexpr int kBlkFinCols = 8;

struct BlkLane {
    int cu;      // the lane's group of 8 columns within a block
    int p, P;    // position among the workgroup's walkers
    bool on;
};
__device__ __forceinline__ BlkLane blk_lane(int F, int cw) {
    BlkLane l;
    l.P = kThreads / cw;
    l.p = threadIdx.x / cw;
    l.cu = blockIdx.x * kThreads + threadIdx.x % cw;
    l.on = l.p < l.P && l.cu < F / 8;
    return l;
}

// the positions' sums of a column, added in position order; part[(2 chunk + k) * F + col]. The LDS
// image is [e][thread]: a lane stores 8 bytes beside its neighbour's (no bank conflict on the
// stores), and the adding lanes j = e cw + c read consecutive doubles within one e. Rows of the
// image lie 2048 bytes apart, so with cw < 32 the e groups of a wave share banks (cw = 8, F = 64:
// 8-way on each of the 2 x 32 reads): 64 LDS reads per adding lane beside 80 global loads per
// lane of the walk, not worth a padded image.
__device__ __forceinline__ void blk_reduce_store(double (&s0)[8], double (&s1)[8], double *part, int F, int cw) {
    __shared__ double red[8][kThreads];
    const int P = kThreads / cw;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[e][threadIdx.x] = k ? s1[e] : s0[e];
        __syncthreads();
        for (int j = threadIdx.x; j < cw * 8; j += kThreads) {
            const int c = j % cw, e = j / cw;
            const int col = (blockIdx.x * kThreads + c) * 8 + e;
            if (col < F) {
                double t = red[e][c];
                for (int p = 1; p < P; ++p) t += red[e][p * cw + c];
                part[((long long)blockIdx.y * 2 + k) * F + col] = t;
            }
        }
        __syncthreads();
    }
}

// the positions' counts of a column (kf_bn_block_stats_relu), added in position order; cnt[chunk * F + col]
__device__ __forceinline__ void blk_reduce_store_count(const int (&n)[8], unsigned *cnt, int F, int cw) {
    __shared__ int redn[8][kThreads];
    const int P = kThreads / cw;
#pragma unroll
    for (int e = 0; e < 8; ++e) redn[e][threadIdx.x] = n[e];
    __syncthreads();
    for (int j = threadIdx.x; j < cw * 8; j += kThreads) {
        const int c = j % cw, e = j / cw;
        const int col = (blockIdx.x * kThreads + c) * 8 + e;
        if (col < F) {
            int t = redn[e][c];
            for (int p = 1; p < P; ++p) t += redn[e][p * cw + c];
            cnt[(long long)blockIdx.y * F + col] = (unsigned)t;
        }
    }
}

// COUNT (k_bnb_fwd_part_relu only): also the number of elements r > 0; false is the kernel as it was
template <bool COUNT>
__device__ __forceinline__ void bnb_fwd_part_body(const h16 *r, long long ld, int rows, int H, int F, int cw, double *part,
                                                  unsigned *cnt) {
    const BlkLane l = blk_lane(F, cw);
    const int r0 = blockIdx.y * kBlkRows, r1 = min(rows, r0 + kBlkRows);
    double s0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (l.on) {
        const long long nq = (long long)(r1 - r0) * H;  // block rows of this workgroup
        const int dr = l.P / H, dh = l.P % H;
        int row = r0 + l.p / H, h = l.p % H;
        const h16 *base = r + (long long)l.cu * 8;
#pragma unroll 4
        for (long long q = l.p; q < nq; q += l.P) {
            const half8 v = load_h8(base + (long long)row * ld + (long long)h * F);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double x = (double)h2f(v[e]);
                s0[e] += x;
                s1[e] = fma(x, x, s1[e]);
                if constexpr (COUNT) n[e] += x > 0.0 ? 1 : 0;
            }
            row += dr;
            h += dh;
            if (h >= H) h -= H, ++row;
        }
    }
    blk_reduce_store(s0, s1, part, F, cw);
    if constexpr (COUNT) blk_reduce_store_count(n, cnt, F, cw);
}
__global__ __launch_bounds__(kThreads) void k_bnb_fwd_part(const h16 *r, long long ld, int rows, int H, int F, int cw,
                                                           double *part) {
    bnb_fwd_part_body<false>(r, ld, rows, H, F, cw, part, nullptr);
}
__global__ __launch_bounds__(kThreads) void k_bnb_fwd_part_relu(const h16 *r, long long ld, int rows, int H, int F, int cw,
                                                                double *part, unsigned *cnt) {
    bnb_fwd_part_body<true>(r, ld, rows, H, F, cw, part, cnt);
}

__global__ __launch_bounds__(kThreads) void k_bnb_bwd_part(const h16 *g, long long ldg, const h16 *r, long long ldr,
                                                           int rows, int H, int F, int cw, double *part) {
    const BlkLane l = blk_lane(F, cw);
    const int r0 = blockIdx.y * kBlkRows, r1 = min(rows, r0 + kBlkRows);
    double s0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (l.on) {
        const long long nq = (long long)(r1 - r0) * H;
        const int dr = l.P / H, dh = l.P % H;
        int row = r0 + l.p / H, h = l.p % H;
        const h16 *gbase = g + (long long)l.cu * 8, *rbase = r + (long long)l.cu * 8;
#pragma unroll 2
        for (long long q = l.p; q < nq; q += l.P) {
            const long long hf = (long long)h * F;
            const half8 gv = load_h8(gbase + (long long)row * ldg + hf);
            const half8 rv = load_h8(rbase + (long long)row * ldr + hf);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double dy = (double)h2f(gv[e]);
                s0[e] += dy;
                s1[e] = fma(dy, (double)h2f(rv[e]), s1[e]);
            }
            row += dr;
            h += dh;
            if (h >= H) h -= H, ++row;
        }
    }
    blk_reduce_store(s0, s1, part, F, cw);
}

// out = rne_fp16(((r scale + shift) drop) + alpha resid): the fused epilogue's fp32 operations in
// its order (gemm_common.h epilogue8: fmaf, multiply, fmaf). Thread = 8 columns of one row.
__global__ __launch_bounds__(kThreads) void k_bn_fwd_apply(const h16 *r, long long ld, long long units, int d8,
                                                           const float *scale, const float *shift, Drop dr,
                                                           const h16 *resid, long long ldres, float alpha, h16 *out,
                                                           long long ldo) {
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= units) return;
    const long long m = u / d8;
    const int c0 = (int)(u - m * d8) * 8;
    const half8 rv = load_h8(r + m * ld + c0);
    float sc[8], sh[8], v[8];
    load_f8(scale + c0, sc);
    load_f8(shift + c0, sh);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = fmaf(h2f(rv[e]), sc[e], sh[e]);
    if (dr.tab) {
        float d[8];
        load_f8(dr.tab + (long long)dr.row_seg[m] * dr.ld + c0, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= d[e];
    }
    if (resid) {
        const half8 x = load_h8(resid + m * ldres + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaf(alpha, h2f(x[e]), v[e]);
    }
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2h(v[e]);
    store_h8(out + m * ldo + c0, o);
}

// dz = rne_fp16(scale (dy - a - yhat b) relu_bit), in double up to the store. Thread = 8 columns of
// kApplyRows consecutive rows, so that the columns' constants are made once for them:
// scale (dy - a - yhat b) = scale dy - k1 r - k0 with k1 = scale^2 b / rms, k0 = scale (a + b shift / rms)
// MASK false: a BatchNorm with no ReLU below it (relu_bit = 1), no mask read. Its eight ones arrive
// as data, in the argument `ones` (0xFF from the host; the masked variants ignore it): with a
// constant the compiler drops the select in front of the store and then rounds every element
// double -> float -> half, where the masked variant's code rounds two of each eight columns
// double -> half in one step. Fed as data, both variants compile to the same
// arithmetic and agree bit for bit under an all-ones mask. That rests on the compiler, not on the
// source, and tests/test_gpu_bn_block.py is what guards it; one explicit rounding order for both
// variants would change the masked path's bits and is a change of its own.
//
// ROWS (kf_bn_train_bwd_apply_rows): the statistics were those of the first stat_rows
// rows only, so the rows from stat_rows on take dz = rne_fp16(scale dy relu_bit), no correction. The
// threshold is a property of the row, one branch per row that all but the wave on the threshold
// takes one way (a first version, selects on r and k0 per element in one fma chain, was bound by
// its double-precision selects); the columns' constants are still made once for the
// four rows, and a group of four may straddle stat_rows. ROWS false is the code
// the kernel always was (stat_rows unused), under the symbol it always had (k_bn_bwd_apply), so
// kf_bn_train_bwd_apply's bits cannot move; k_bn_bwd_apply_rows is the body with the threshold.
constexpr int kApplyRows = 4;
template <bool DROP, bool MASK, bool ROWS, bool REPAIR = false>
__device__ __forceinline__ void bn_bwd_apply_body(const h16 *g, long long ldg, const h16 *r, long long ldr, int rows,
                                                  int stat_rows, long long units, int d8, const float *scale,
                                                  const float *shift, double inv_rms, const float *a, const float *b,
                                                  Drop dr, const uint8_t *mask, long long ld_mask, h16 *dz, long long lddz,
                                                  unsigned ones, const float *repair = nullptr) {
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= units) return;
    const long long grp = u / d8;
    const int c0 = (int)(u - grp * d8) * 8;
    // REPAIR (k_bn_bwd_apply_repair, behind the plain kernel on the stream): the columns whose
    // self-repair term is not zero are evaluated again with the term inside the one rounding, and
    // an element whose relu_bit is 0 stores the term alone. Every other column keeps the bits the
    // plain kernel stored (how that kernel rounds a column rests on the compiler, see MASK above:
    // nothing here may stand in for it), and a group of 8 columns without a term is not touched: its
    // lanes load the 32 bytes of the term and return, before any other load.
    double sr[8];
    bool nz[8];
    if constexpr (REPAIR) {
        float s[8];
        load_f8(repair + c0, s);
        bool any = false;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sr[e] = (double)s[e];
            nz[e] = s[e] != 0.f;
            any = any || nz[e];
        }
        if (!any) return;
    }
    float sc[8], sh[8], av[8], bv[8];
    load_f8(scale + c0, sc);
    load_f8(shift + c0, sh);
    load_f8(a + c0, av);
    load_f8(b + c0, bv);
    double scd[8], k1[8], k0[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        scd[e] = (double)sc[e];
        const double sb = scd[e] * (double)bv[e] * inv_rms;
        k1[e] = sb * scd[e];
        k0[e] = fma(sb, (double)sh[e], scd[e] * (double)av[e]);
    }
    const long long m0 = grp * kApplyRows;
#pragma unroll
    for (int i = 0; i < kApplyRows; ++i) {
        const long long m = m0 + i;
        if (m >= rows) break;
        const half8 gv = load_h8(g + m * ldg + c0), rv = load_h8(r + m * ldr + c0);
        unsigned bits = ones;  // (MASK false: all ones, as data, see above)
        if constexpr (MASK) bits = mask[(m * ld_mask + c0) >> 3];
        float d[8];
        if constexpr (DROP) load_f8(dr.tab + (long long)dr.row_seg[m] * dr.ld + c0, d);
        half8 o;
        if (!ROWS || m < stat_rows) {  // (per row: the same for its 8 columns and for every lane on the row)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                double dy = (double)h2f(gv[e]);
                if constexpr (DROP) dy *= (double)d[e];
                const double w = fma(scd[e], dy, -fma(k1[e], (double)h2f(rv[e]), k0[e]));
                if constexpr (REPAIR) o[e] = f2h((float)((((bits >> e) & 1u) ? w : 0.0) + sr[e]));
                else o[e] = ((bits >> e) & 1u) ? f2h((float)w) : (h16)0.f;
            }
            if constexpr (REPAIR) {
                const half8 plain = load_h8(dz + m * lddz + c0);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = nz[e] ? o[e] : plain[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                double dy = (double)h2f(gv[e]);
                if constexpr (DROP) dy *= (double)d[e];
                o[e] = ((bits >> e) & 1u) ? f2h((float)(scd[e] * dy)) : (h16)0.f;
            }
        }
        store_h8(dz + m * lddz + c0, o);
    }
}
template <bool DROP, bool MASK>
__global__ __launch_bounds__(kThreads) void k_bn_bwd_apply(const h16 *g, long long ldg, const h16 *r, long long ldr,
                                                           int rows, long long units, int d8, const float *scale,
                                                           const float *shift, double inv_rms, const float *a,
                                                           const float *b, Drop dr, const uint8_t *mask,
                                                           long long ld_mask, h16 *dz, long long lddz, unsigned ones) {
    bn_bwd_apply_body<DROP, MASK, false>(g, ldg, r, ldr, rows, rows, units, d8, scale, shift, inv_rms, a, b, dr, mask, ld_mask,
                                         dz, lddz, ones);
}
template <bool DROP, bool MASK>
__global__ __launch_bounds__(kThreads) void k_bn_bwd_apply_rows(const h16 *g, long long ldg, const h16 *r, long long ldr,
                                                                int rows, int stat_rows, long long units, int d8,
                                                                const float *scale, const float *shift, double inv_rms,
                                                                const float *a, const float *b, Drop dr,
                                                                const uint8_t *mask, long long ld_mask, h16 *dz,
                                                                long long lddz, unsigned ones) {
    bn_bwd_apply_body<DROP, MASK, true>(g, ldg, r, ldr, rows, stat_rows, units, d8, scale, shift, inv_rms, a, b, dr, mask,
                                        ld_mask, dz, lddz, ones);
}

// kf_bn_train_bwd_apply_repair / _rows_repair: the body above with the repair term,
// over the statistics rows and the columns with a term only, behind the plain kernel (bwd_apply
// below); kernels of their own, so the eight above keep their code.
template <bool DROP, bool MASK>
__global__ __launch_bounds__(kThreads) void k_bn_bwd_apply_repair(const h16 *g, long long ldg, const h16 *r, long long ldr,
                                                                  int rows, long long units, int d8, const float *scale,
                                                                  const float *shift, double inv_rms, const float *a,
                                                                  const float *b, Drop dr, const uint8_t *mask,
                                                                  long long ld_mask, h16 *dz, long long lddz, unsigned ones,
                                                                  const float *repair) {
    bn_bwd_apply_body<DROP, MASK, false, true>(g, ldg, r, ldr, rows, rows, units, d8, scale, shift, inv_rms, a, b, dr, mask,
                                               ld_mask, dz, lddz, ones, repair);
}

// s = -k S, +k S or 0 per column of every site of a backward (kf_relu_repair_vectors):
// blockIdx.y = site, a lane = 4 columns, the comparisons in double. D % 4 == 0 (the entry checks
// D % 8), s 16-byte aligned: one 16-byte vector store per lane.
__global__ __launch_bounds__(kThreads) void k_relu_repair_vectors(const KfRepairSite *sites, const float *loss_scale) {
    const KfRepairSite st = sites[blockIdx.y];
    const int c0 = (blockIdx.x * kThreads + threadIdx.x) * 4;
    if (c0 >= st.D) return;
    const double count = st.count[0];
    const float ks = st.scale * (loss_scale ? loss_scale[0] : 1.f);
    const double lo = (double)st.lower * count, hi = (double)st.upper * count;
    float4v o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double d = st.deriv[c0 + e];
        o[e] = count == 0.0 ? 0.f : d <= lo ? -ks : d > hi ? ks : 0.f;
    }
    *reinterpret_cast<float4v *>(st.s + c0) = o;
}

bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// shape rules shared by the four entries: rows x D fp16 tensors read with 16-byte lanes
bool shape_ok(const char *what, int rows, int D) {
    if (rows > 0 && rows <= 65535 * kChunk && D > 0 && D % 8 == 0) return true;
    kf_report_error("%s: needs 0 < rows <= %d, D > 0 and D %% 8 == 0 (rows=%d D=%d)", what, 65535 * kChunk, rows, D);
    return false;
}
bool tensor_ok(const char *what, const char *name, const void *p, long long ld, int D) {
    if (p && al16(p) && ld >= D && ld % 8 == 0) return true;
    kf_report_error("%s: %s needs a 16-byte aligned pointer and ld >= D, ld %% 8 == 0 (ld=%lld D=%d)", what, name, ld, D);
    return false;
}
bool cols_ok(const char *what, const char *name, const float *p) {
    if (p && al16(p)) return true;
    kf_report_error("%s: %s needs a 16-byte aligned pointer", what, name);
    return false;
}
bool drop_ok(const char *what, const float *drop, long long ld_drop, const int32_t *row_seg, int D) {
    if (!drop) return true;
    if (row_seg && al16(drop) && ld_drop >= D && ld_drop % 4 == 0) return true;
    kf_report_error("%s: drop needs row_seg, a 16-byte aligned table and ld_drop >= D, ld_drop %% 4 == 0", what);
    return false;
}
bool launched(const char *what) {
    if (hipGetLastError() == hipSuccess) return true;
    kf_report_error("%s: launch failed", what);
    return false;
}
int chunks_of(int rows) { return (rows + kChunk - 1) / kChunk; }
// planes = 3: room for the _relu entries' counts (unsigned, half of the third plane) behind the sums
double *partials(const char *what, int rows, int D, int planes = 2) {
    double *p = (double *)kf_workspace_stream((size_t)chunks_of(rows) * planes * D * sizeof(double));
    if (!p) kf_report_error("%s: workspace", what);
    return p;
}

}  // namespace

namespace {

// the ReLU statistics of the _relu entries: both or none
bool relu_acc_ok(const char *what, const double *relu_count, const double *relu_deriv) {
    if (!relu_count == !relu_deriv) return true;
    kf_report_error("%s: needs relu_count and relu_deriv, or neither", what);
    return false;
}

// kf_bn_train_stats / _relu. relu_deriv == NULL launches the two kernels kf_bn_train_stats always
// launched; else the counting pair, whose count partials lie behind the sums' in the scratch.
int fwd_stats(const char *what, const void *r, long long ld, int rows, int D, float eps, float target_rms, float *mean, float *var,
              float *scale, float *shift, double *acc_count, double *acc_sum, double *acc_sumsq, double *relu_count,
              double *relu_deriv) {
    if (!shape_ok(what, rows, D) || !tensor_ok(what, "r", r, ld, D) || !relu_acc_ok(what, relu_count, relu_deriv)) return -1;
    if (!mean || !var || !scale || !shift || !(eps >= 0.f) || !(target_rms > 0.f) ||
        ((acc_count || acc_sum || acc_sumsq) && !(acc_count && acc_sum && acc_sumsq))) {
        kf_report_error("%s: needs mean, var, scale, shift, eps >= 0, target_rms > 0 and all three accumulators or none", what);
        return -1;
    }
    const int nchunk = chunks_of(rows);
    double *part = partials(what, rows, D, relu_deriv ? 3 : 2);
    if (!part) return -1;
    const dim3 grid((unsigned)((D + kSlab - 1) / kSlab), (unsigned)nchunk);
    const unsigned fin = (unsigned)((D + kFinCols - 1) / kFinCols);
    if (relu_deriv) {
        unsigned *cnt = (unsigned *)(part + (size_t)nchunk * 2 * D);
        k_bn_fwd_part_relu<<<grid, kThreads, 0, kf_stream()>>>((const h16 *)r, ld, rows, D, part, cnt);
        k_bn_fwd_finish_relu<kFinCols><<<fin, kThreads, 0, kf_stream()>>>(part, nchunk, (double)rows, D, (double)eps,
                                                                          (double)target_rms, mean, var, scale, shift, acc_count,
                                                                          acc_sum, acc_sumsq, cnt, relu_count, relu_deriv);
        return launched(what) ? 0 : -1;
    }
    k_bn_fwd_part<<<grid, kThreads, 0, kf_stream()>>>((const h16 *)r, ld, rows, D, part);
    k_bn_fwd_finish<kFinCols><<<fin, kThreads, 0, kf_stream()>>>(part, nchunk, (double)rows, D, (double)eps, (double)target_rms,
                                                                 mean, var, scale, shift, acc_count, acc_sum, acc_sumsq);
    return launched(what) ? 0 : -1;
}

}  // namespace

extern "C" int kf_bn_train_stats(const void *r, long long ld, int rows, int D, float eps, float target_rms, float *mean,
                                 float *var, float *scale, float *shift, double *acc_count, double *acc_sum,
                                 double *acc_sumsq) {
    kf_take_pending(__func__);
    return fwd_stats("kf_bn_train_stats", r, ld, rows, D, eps, target_rms, mean, var, scale, shift, acc_count, acc_sum, acc_sumsq,
                     nullptr, nullptr);
}

extern "C" int kf_bn_train_stats_relu(const void *r, long long ld, int rows, int D, float eps, float target_rms, float *mean,
                                      float *var, float *scale, float *shift, double *acc_count, double *acc_sum,
                                      double *acc_sumsq, double *relu_count, double *relu_deriv) {
    kf_take_pending(__func__);
    return fwd_stats("kf_bn_train_stats_relu", r, ld, rows, D, eps, target_rms, mean, var, scale, shift, acc_count, acc_sum,
                     acc_sumsq, relu_count, relu_deriv);
}

extern "C" int kf_bn_train_apply(const void *r, long long ld, int rows, int D, const float *scale, const float *shift,
                                 const float *drop, long long ld_drop, const int32_t *row_seg, const void *resid,
                                 long long ldr, float alpha, void *out, long long ldo) {
    kf_take_pending(__func__);
    const char *what = "kf_bn_train_apply";
    if (!shape_ok(what, rows, D) || !tensor_ok(what, "r", r, ld, D) || !tensor_ok(what, "out", out, ldo, D) ||
        !cols_ok(what, "scale", scale) || !cols_ok(what, "shift", shift) || !drop_ok(what, drop, ld_drop, row_seg, D) ||
        (resid && !tensor_ok(what, "resid", resid, ldr, D)))
        return -1;
    const int d8 = D / 8;
    const long long units = (long long)rows * d8;
    k_bn_fwd_apply<<<(unsigned)((units + kThreads - 1) / kThreads), kThreads, 0, kf_stream()>>>(
        (const h16 *)r, ld, units, d8, scale, shift, Drop{drop, ld_drop, row_seg}, (const h16 *)resid, ldr, alpha,
        (h16 *)out, ldo);
    return launched(what) ? 0 : -1;
}

namespace {

// kf_bn_train_bwd_stats / _rows: the sums over `rows`, the divisor stat_rows
int bwd_stats(const char *what, const void *g, long long ldg, const void *r, long long ldr, int rows, int stat_rows, int D,
              const float *scale, const float *shift, float target_rms, const float *drop, long long ld_drop,
              const int32_t *row_seg, float *a, float *b) {
    if (!shape_ok(what, rows, D) || !tensor_ok(what, "g", g, ldg, D) || !tensor_ok(what, "r", r, ldr, D) ||
        !drop_ok(what, drop, ld_drop, row_seg, D))
        return -1;
    if (!scale || !shift || !a || !b || !(target_rms > 0.f)) {
        kf_report_error("%s: needs scale, shift, a, b and target_rms > 0", what);
        return -1;
    }
    if (stat_rows < 1 || stat_rows > rows) {
        kf_report_error("%s: needs 1 <= stat_rows <= rows (stat_rows=%d rows=%d)", what, stat_rows, rows);
        return -1;
    }
    double *part = partials(what, rows, D);
    if (!part) return -1;
    const int nchunk = chunks_of(rows);
    const dim3 grid((unsigned)((D + kSlab - 1) / kSlab), (unsigned)nchunk);
    const Drop dr{drop, ld_drop, row_seg};
    if (drop) k_bn_bwd_part<true><<<grid, kThreads, 0, kf_stream()>>>((const h16 *)g, ldg, (const h16 *)r, ldr, rows, D, dr, part);
    else k_bn_bwd_part<false><<<grid, kThreads, 0, kf_stream()>>>((const h16 *)g, ldg, (const h16 *)r, ldr, rows, D, dr, part);
    k_bn_bwd_finish<kFinCols><<<(unsigned)((D + kFinCols - 1) / kFinCols), kThreads, 0, kf_stream()>>>(
        part, nchunk, (double)stat_rows, D, scale, shift, 1.0 / (double)target_rms, a, b);
    return launched(what) ? 0 : -1;
}

// kf_bn_train_bwd_apply / _rows. stat_rows == rows launches the kernel without the row threshold,
// the one kf_bn_train_bwd_apply always launched.
int bwd_apply(const char *what, const void *g, long long ldg, const void *r, long long ldr, int rows, int stat_rows, int D,
              const float *scale, const float *shift, float target_rms, const float *a, const float *b, const float *drop,
              long long ld_drop, const int32_t *row_seg, const uint8_t *mask, long long ld_mask, void *dz, long long lddz,
              const float *repair = nullptr) {
    if (!shape_ok(what, rows, D) || !tensor_ok(what, "g", g, ldg, D) || !tensor_ok(what, "r", r, ldr, D) ||
        !tensor_ok(what, "dz", dz, lddz, D) || !cols_ok(what, "scale", scale) || !cols_ok(what, "shift", shift) ||
        !cols_ok(what, "a", a) || !cols_ok(what, "b", b) || !drop_ok(what, drop, ld_drop, row_seg, D) ||
        (repair && !cols_ok(what, "repair", repair)))
        return -1;
    if ((mask && (ld_mask < D || ld_mask % 8)) || !(target_rms > 0.f)) {
        kf_report_error("%s: needs the ReLU mask with ld_mask >= D bits, ld_mask %% 8 == 0 (or none), and target_rms > 0", what);
        return -1;
    }
    if (stat_rows < 1 || stat_rows > rows) {
        kf_report_error("%s: needs 1 <= stat_rows <= rows (stat_rows=%d rows=%d)", what, stat_rows, rows);
        return -1;
    }
    if (repair && (dz == g || dz == r)) {  // (the second launch reads g and r again behind the first one's stores)
        kf_report_error("%s: dz may not alias g or r", what);
        return -1;
    }
    const int d8 = D / 8;
    const long long units = (long long)((rows + kApplyRows - 1) / kApplyRows) * d8;
    const unsigned nblk = (unsigned)((units + kThreads - 1) / kThreads);
    const Drop dr{drop, ld_drop, row_seg};
    const double inv_rms = 1.0 / (double)target_rms;
#define KF_BN_BWD_APPLY(KERNEL, ...)                                                                                   \
    KERNEL<<<nblk, kThreads, 0, kf_stream()>>>((const h16 *)g, ldg, (const h16 *)r, ldr, rows, __VA_ARGS__ units, d8, scale, \
                                               shift, inv_rms, a, b, dr, mask, ld_mask, (h16 *)dz, lddz, 0xFFu)
    if (stat_rows < rows) {
        if (drop && mask) KF_BN_BWD_APPLY((k_bn_bwd_apply_rows<true, true>), stat_rows, );
        else if (mask) KF_BN_BWD_APPLY((k_bn_bwd_apply_rows<false, true>), stat_rows, );
        else if (drop) KF_BN_BWD_APPLY((k_bn_bwd_apply_rows<true, false>), stat_rows, );
        else KF_BN_BWD_APPLY((k_bn_bwd_apply_rows<false, false>), stat_rows, );
    } else {
        if (drop && mask) KF_BN_BWD_APPLY((k_bn_bwd_apply<true, true>), );
        else if (mask) KF_BN_BWD_APPLY((k_bn_bwd_apply<false, true>), );
        else if (drop) KF_BN_BWD_APPLY((k_bn_bwd_apply<true, false>), );
        else KF_BN_BWD_APPLY((k_bn_bwd_apply<false, false>), );
    }
#undef KF_BN_BWD_APPLY
    if (repair) {
        // the plain kernel above wrote every row; the columns with a term again, on the statistics rows
        const long long sunits = (long long)((stat_rows + kApplyRows - 1) / kApplyRows) * d8;
        const unsigned sblk = (unsigned)((sunits + kThreads - 1) / kThreads);
#define KF_BN_BWD_REPAIR(DROP, MASK)                                                                                        \
    k_bn_bwd_apply_repair<DROP, MASK><<<sblk, kThreads, 0, kf_stream()>>>((const h16 *)g, ldg, (const h16 *)r, ldr, stat_rows,    \
                                                                          sunits, d8, scale, shift, inv_rms, a, b, dr, mask,     \
                                                                          ld_mask, (h16 *)dz, lddz, 0xFFu, repair)
        if (drop && mask) KF_BN_BWD_REPAIR(true, true);
        else if (mask) KF_BN_BWD_REPAIR(false, true);
        else if (drop) KF_BN_BWD_REPAIR(true, false);
        else KF_BN_BWD_REPAIR(false, false);
#undef KF_BN_BWD_REPAIR
    }
    return launched(what) ? 0 : -1;
}

}  // namespace

extern "C" int kf_bn_train_bwd_stats(const void *g, long long ldg, const void *r, long long ldr, int rows, int D,
                                     const float *scale, const float *shift, float target_rms, const float *drop,
                                     long long ld_drop, const int32_t *row_seg, float *a, float *b) {
    kf_take_pending(__func__);
    return bwd_stats("kf_bn_train_bwd_stats", g, ldg, r, ldr, rows, rows, D, scale, shift, target_rms, drop, ld_drop, row_seg, a,
                     b);
}

extern "C" int kf_bn_train_bwd_stats_rows(const void *g, long long ldg, const void *r, long long ldr, int rows, int stat_rows,
                                          int D, const float *scale, const float *shift, float target_rms, const float *drop,
                                          long long ld_drop, const int32_t *row_seg, float *a, float *b) {
    kf_take_pending(__func__);
    return bwd_stats("kf_bn_train_bwd_stats_rows", g, ldg, r, ldr, rows, stat_rows, D, scale, shift, target_rms, drop, ld_drop,
                     row_seg, a, b);
}

extern "C" int kf_bn_train_bwd_apply(const void *g, long long ldg, const void *r, long long ldr, int rows, int D,
                                     const float *scale, const float *shift, float target_rms, const float *a,
                                     const float *b, const float *drop, long long ld_drop, const int32_t *row_seg,
                                     const uint8_t *mask, long long ld_mask, void *dz, long long lddz) {
    kf_take_pending(__func__);
    return bwd_apply("kf_bn_train_bwd_apply", g, ldg, r, ldr, rows, rows, D, scale, shift, target_rms, a, b, drop, ld_drop,
                     row_seg, mask, ld_mask, dz, lddz);
}

extern "C" int kf_bn_train_bwd_apply_rows(const void *g, long long ldg, const void *r, long long ldr, int rows, int stat_rows,
                                          int D, const float *scale, const float *shift, float target_rms, const float *a,
                                          const float *b, const float *drop, long long ld_drop, const int32_t *row_seg,
                                          const uint8_t *mask, long long ld_mask, void *dz, long long lddz) {
    kf_take_pending(__func__);
    return bwd_apply("kf_bn_train_bwd_apply_rows", g, ldg, r, ldr, rows, stat_rows, D, scale, shift, target_rms, a, b, drop,
                     ld_drop, row_seg, mask, ld_mask, dz, lddz);
}

extern "C" int kf_bn_train_bwd_apply_repair(const void *g, long long ldg, const void *r, long long ldr, int rows, int D,
                                            const float *scale, const float *shift, float target_rms, const float *a,
                                            const float *b, const float *drop, long long ld_drop, const int32_t *row_seg,
                                            const uint8_t *mask, long long ld_mask, void *dz, long long lddz,
                                            const float *repair) {
    kf_take_pending(__func__);
    return bwd_apply("kf_bn_train_bwd_apply_repair", g, ldg, r, ldr, rows, rows, D, scale, shift, target_rms, a, b, drop, ld_drop,
                     row_seg, mask, ld_mask, dz, lddz, repair);
}

extern "C" int kf_bn_train_bwd_apply_rows_repair(const void *g, long long ldg, const void *r, long long ldr, int rows,
                                                 int stat_rows, int D, const float *scale, const float *shift, float target_rms,
                                                 const float *a, const float *b, const float *drop, long long ld_drop,
                                                 const int32_t *row_seg, const uint8_t *mask, long long ld_mask, void *dz,
                                                 long long lddz, const float *repair) {
    kf_take_pending(__func__);
    return bwd_apply("kf_bn_train_bwd_apply_rows_repair", g, ldg, r, ldr, rows, stat_rows, D, scale, shift, target_rms, a, b, drop,
                     ld_drop, row_seg, mask, ld_mask, dz, lddz, repair);
}

extern "C" int kf_relu_repair_vectors(const KfRepairSite *sites, const KfRepairSite *sites_dev, int n,
                                      const float *loss_scale_dev) {
    kf_take_pending(__func__);
    const char *what = "kf_relu_repair_vectors";
    if (!sites || !sites_dev || n < 1 || n > 65535) {
        kf_report_error("%s: needs the table on the host and on the device and 1 <= n <= 65535 (n=%d)", what, n);
        return -1;
    }
    int maxd = 0;
    for (int i = 0; i < n; ++i) {
        const KfRepairSite &s = sites[i];
        if (!s.count || !s.deriv || !s.s || !al16(s.s) || s.D <= 0 || s.D % 8 || !(s.scale >= 0.f) ||
            !(s.lower >= 0.f && s.lower < s.upper && s.upper <= 1.f)) {
            kf_report_error("%s: site %d needs count, deriv, a 16-byte aligned s, D > 0, D %% 8 == 0, scale >= 0 and "
                            "0 <= lower < upper <= 1 (D=%d)", what, i, s.D);
            return -1;
        }
        maxd = std::max(maxd, s.D);
    }
    const dim3 grid((unsigned)((maxd / 4 + kThreads - 1) / kThreads), (unsigned)n);
    k_relu_repair_vectors<<<grid, kThreads, 0, kf_stream()>>>(sites_dev, loss_scale_dev);
    return launched(what) ? 0 : -1;
}

// ---- block statistics: the entries ----
namespace {

// r [rows x H F] read with 16-byte lanes, statistics [F]
bool block_shape_ok(const char *what, int rows, int H, int F) {
    if (rows > 0 && rows <= 65535 * kBlkRows && H >= 1 && F > 0 && F % 8 == 0 && (long long)H * F <= 0x7fffffffll) return true;
    kf_report_error("%s: needs 0 < rows <= %d, H >= 1, F > 0 and F %% 8 == 0 (rows=%d H=%d F=%d)", what, 65535 * kBlkRows, rows,
                    H, F);
    return false;
}
bool block_tensor_ok(const char *what, const char *name, const void *p, long long ld, int H, int F) {
    if (p && al16(p) && ld >= (long long)H * F && ld % 8 == 0) return true;
    kf_report_error("%s: %s needs a 16-byte aligned pointer and ld >= H F, ld %% 8 == 0 (ld=%lld H=%d F=%d)", what, name, ld, H,
                    F);
    return false;
}
int block_chunks(int rows) { return (rows + kBlkRows - 1) / kBlkRows; }
int block_cw(int F) { return std::min(F / 8, kThreads); }
dim3 block_grid(int rows, int F) { return dim3((unsigned)((F / 8 + kThreads - 1) / kThreads), (unsigned)block_chunks(rows)); }
double *block_partials(const char *what, int rows, int F, int planes = 2) {
    double *p = (double *)kf_workspace_stream((size_t)block_chunks(rows) * planes * F * sizeof(double));
    if (!p) kf_report_error("%s: workspace", what);
    return p;
}

}  // namespace

namespace {

// kf_bn_block_stats / _relu, as fwd_stats above
int block_fwd_stats(const char *what, const void *r, long long ld, int rows, int H, int F, float eps, float target_rms,
                    float *mean, float *var, float *scale, float *shift, double *acc_count, double *acc_sum, double *acc_sumsq,
                    double *relu_count, double *relu_deriv) {
    if (!block_shape_ok(what, rows, H, F) || !block_tensor_ok(what, "r", r, ld, H, F) ||
        !relu_acc_ok(what, relu_count, relu_deriv))
        return -1;
    if (!mean || !var || !scale || !shift || !(eps >= 0.f) || !(target_rms > 0.f) ||
        ((acc_count || acc_sum || acc_sumsq) && !(acc_count && acc_sum && acc_sumsq))) {
        kf_report_error("%s: needs mean, var, scale, shift, eps >= 0, target_rms > 0 and all three accumulators or none", what);
        return -1;
    }
    const int nchunk = block_chunks(rows);
    double *part = block_partials(what, rows, F, relu_deriv ? 3 : 2);
    if (!part) return -1;
    const unsigned fin = (unsigned)((F + kBlkFinCols - 1) / kBlkFinCols);
    if (relu_deriv) {
        unsigned *cnt = (unsigned *)(part + (size_t)nchunk * 2 * F);
        k_bnb_fwd_part_relu<<<block_grid(rows, F), kThreads, 0, kf_stream()>>>((const h16 *)r, ld, rows, H, F, block_cw(F), part,
                                                                               cnt);
        k_bn_fwd_finish_relu<kBlkFinCols><<<fin, kThreads, 0, kf_stream()>>>(part, nchunk, (double)rows * H, F, (double)eps,
                                                                             (double)target_rms, mean, var, scale, shift,
                                                                             acc_count, acc_sum, acc_sumsq, cnt, relu_count,
                                                                             relu_deriv);
        return launched(what) ? 0 : -1;
    }
    k_bnb_fwd_part<<<block_grid(rows, F), kThreads, 0, kf_stream()>>>((const h16 *)r, ld, rows, H, F, block_cw(F), part);
    k_bn_fwd_finish<kBlkFinCols><<<fin, kThreads, 0, kf_stream()>>>(part, nchunk, (double)rows * H, F, (double)eps,
                                                                    (double)target_rms, mean, var, scale, shift, acc_count,
                                                                    acc_sum, acc_sumsq);
    return launched(what) ? 0 : -1;
}

}  // namespace

extern "C" int kf_bn_block_stats(const void *r, long long ld, int rows, int H, int F, float eps, float target_rms,
                                 float *mean, float *var, float *scale, float *shift, double *acc_count, double *acc_sum,
                                 double *acc_sumsq) {
    kf_take_pending(__func__);
    return block_fwd_stats("kf_bn_block_stats", r, ld, rows, H, F, eps, target_rms, mean, var, scale, shift, acc_count, acc_sum,
                           acc_sumsq, nullptr, nullptr);
}

extern "C" int kf_bn_block_stats_relu(const void *r, long long ld, int rows, int H, int F, float eps, float target_rms,
                                      float *mean, float *var, float *scale, float *shift, double *acc_count, double *acc_sum,
                                      double *acc_sumsq, double *relu_count, double *relu_deriv) {
    kf_take_pending(__func__);
    return block_fwd_stats("kf_bn_block_stats_relu", r, ld, rows, H, F, eps, target_rms, mean, var, scale, shift, acc_count,
                           acc_sum, acc_sumsq, relu_count, relu_deriv);
}

extern "C" int kf_bn_block_bwd_stats(const void *g, long long ldg, const void *r, long long ldr, int rows, int H, int F,
                                     const float *scale, const float *shift, float target_rms, float *a, float *b) {
    kf_take_pending(__func__);
    const char *what = "kf_bn_block_bwd_stats";
    if (!block_shape_ok(what, rows, H, F) || !block_tensor_ok(what, "g", g, ldg, H, F) ||
        !block_tensor_ok(what, "r", r, ldr, H, F))
        return -1;
    if (!scale || !shift || !a || !b || !(target_rms > 0.f)) {
        kf_report_error("%s: needs scale, shift, a, b and target_rms > 0", what);
        return -1;
    }
    double *part = block_partials(what, rows, F);
    if (!part) return -1;
    k_bnb_bwd_part<<<block_grid(rows, F), kThreads, 0, kf_stream()>>>((const h16 *)g, ldg, (const h16 *)r, ldr, rows, H, F,
                                                                     block_cw(F), part);
    k_bn_bwd_finish<kBlkFinCols><<<(unsigned)((F + kBlkFinCols - 1) / kBlkFinCols), kThreads, 0, kf_stream()>>>(
        part, block_chunks(rows), (double)rows * H, F, scale, shift, 1.0 / (double)target_rms, a, b);
    return launched(what) ? 0 : -1;
}
