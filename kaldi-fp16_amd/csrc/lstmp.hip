// lstmp.hip — Kaldi's projected LSTM (fast-lstmp-layer) as a sequence operator: forward and exact
// backward (include/kf_lstm.h).
//
// One launch per kernel and recurrence step, ordered by the stream only: no workgroup waits on
// another one, no atomics, every sum in a fixed order, so a call replays bit for bit. Step s covers
// frames [s |d|, (s+1) |d|) of every sequence; they depend on step s-1 only, so a step's rows (up to
// B |d|) are independent and are gathered through a row table built on the device once per call.
//
//   forward   k_lstmp_prep, kf_gemm_fused (G = X W_x + b), then per step
//             k_lstmp_step_fwd  a workgroup owns 32 cells = 4 x 32 gate columns: its W_r slice
//                               [128 x R] in LDS, r' rows as A fragments, v_mfma_f32_16x16x32_f16,
//                               + G, nonlinearity on the accumulators; writes c, m, gates
//             k_lstmp_proj      y = W_p m + b_p for the step's rows, r into the shifted copy rs
//   backward  per step in reverse
//             k_lstmp_dm        prologue: dy + clip(dr) rows (kept for dW_p); dm = (dy + dr) W_p
//             k_lstmp_step_bwd  prologue: clip(dc); nonlinearity derivative; dG and the dc carry
//             k_lstmp_dr        dr[t+d] = dG W_r
//             then kf_gemm_wgrad x 3 (W_x and b, W_r, W_p and b_p), kf_gemm_fused (dX) and the
//             peephole gradients (k_lstmp_peep_part / _finish: column sums in double)
#include <algorithm>
#include <vector>

#include "kf_common.h"
#include "kf_prof.h"
#include "../../include/kf_lstm.h"
#include "../../include/kf_ops.h"

KF_DECLARE_ERR(lstmp)

namespace {
constexpr int kThreads = 256;
constexpr int kSlice = 32;      // cells a step workgroup owns
constexpr int kTilesPerWg = 4;  // 16-row tiles a forward step workgroup covers (2 per wave pair)
constexpr int kPad = 8;         // halves of padding per LDS row: the 16 rows of a fragment read fall in 16 bank groups
constexpr int kHasPrev = 1;     // rinfo: frame t + d exists
constexpr int kHasNext = 2;     // rinfo: frame t - d exists
constexpr int kPeepChunks = 64; // row chunks of the peephole sums
constexpr int kLdsMax = 160 * 1024;

// what the kernels see of an operator
struct LstmpDev {
    int D, C, R, N, ad;  // ad = |delay|
    long long oB, oWr, oPeep, oWp, oBp, total;  // offsets in the flat parameter layout
    // fp16 working copies
    h16 *wx;    // [D x 4C]
    h16 *b;     // [4C]
    h16 *wr;    // [R x 4C]      dr = dG W_r: k = gate column
    h16 *wrT;   // [4C x R]      the forward step: k = r
    h16 *peep;  // [3C] w_ic, w_fc, w_oc
    h16 *wp;    // [C x (R+N)]   dm = dyr W_p: k = output column
    h16 *wpT;   // [(R+N) x C]   the projection: k = cell
    h16 *bp;    // [R+N]
    // what the forward keeps
    h16 *G;      // [rows x 4C] X W_x + b
    h16 *gates;  // [rows x 4C] activations i, f, g, o
    float *c;    // [rows x C]
    h16 *m;      // [rows x C]
    h16 *rs;     // [rows x R]  rs[row of t] = r[t + d], zeros while t + d < 0
    // the backward's
    h16 *dG;     // [rows x 4C] derivative at the gate pre-activations
    h16 *dyr;    // [rows x (R+N)] dy + clipped dr
    float *dr;   // [rows x R]  written once per row by frame t - d
    float *dc;   // [rows x C]  the c carry, written once per row by frame t - d
    float *dm;   // [step rows x C]
    double *part;  // [kPeepChunks x 3C]
    const int *table;  // step rows: table[step_off[s] + q] = row
    const int *rinfo;  // [rows] kHasPrev | kHasNext
    float clip;
};

extern __shared__ __attribute__((aligned(16))) char lstmp_lds[];

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// lay: seq_row0[B+1], step_off[nsteps+1]. Blocks 0 .. B-1: a sequence's row flags and the zero rows
// of rs; block B: the row table, one thread per step, sequences in order within a step.
__global__ __launch_bounds__(kThreads) void k_lstmp_prep(const int *lay, int B, int nsteps, int ad, int R, int *table,
                                                         int *rinfo, h16 *rs) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < B) {
        const int r0 = lay[blockIdx.x], len = lay[blockIdx.x + 1] - r0;
        for (int t = tid; t < len; t += kThreads) rinfo[r0 + t] = (t >= ad ? kHasPrev : 0) | (t + ad < len ? kHasNext : 0);
        const int nz = min(ad, len) * (R / 8);
        const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = tid; i < nz; i += kThreads) store_h8(rs + (size_t)r0 * R + 8 * (size_t)i, z);
        return;
    }
    for (int s = tid; s < nsteps; s += kThreads) {
        int n = lay[B + 1 + s];
        for (int i = 0; i < B; ++i) {
            const int r0 = lay[i], len = lay[i + 1] - r0;
            for (int t = s * ad; t < min(len, (s + 1) * ad); ++t) table[n++] = r0 + t;
        }
    }
}

// fp32 master -> every fp16 working copy, the two transposed ones included
__global__ __launch_bounds__(kThreads) void k_lstmp_cast(LstmpDev P, const float *w32) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P.total) return;
    const h16 v = f2h(w32[i]);
    const int C4 = 4 * P.C, RN = P.R + P.N;
    if (i < P.oB) {
        P.wx[i] = v;
    } else if (i < P.oWr) {
        P.b[i - P.oB] = v;
    } else if (i < P.oPeep) {
        const long long e = i - P.oWr;
        P.wr[e] = v;
        P.wrT[(e % C4) * P.R + e / C4] = v;
    } else if (i < P.oWp) {
        P.peep[i - P.oPeep] = v;
    } else if (i < P.oBp) {
        const long long e = i - P.oWp;
        P.wp[e] = v;
        P.wpT[(e % RN) * P.C + e / RN] = v;
    } else {
        P.bp[i - P.oBp] = v;
    }
}

// Step s of the forward, rows table[off .. off + n). grid (C / 32, ceil(n / 64)).
// LDS: Ws[128][R + 8] halves, local column g * 32 + cl = gate column g * C + j0 + cl.
// Wave w: cells j0 + 16 (w & 1) + (lane & 15), row tiles (w >> 1) + 2 i of the workgroup's four; one
// accumulator per gate, so a lane holds i, f, g, o of the same (row, cell) after the K loop.
__global__ __launch_bounds__(kThreads) void k_lstmp_step_fwd(LstmpDev P, int off, int n) {
    h16 *Ws = (h16 *)lstmp_lds;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int C = P.C, R = P.R, pitch = R + kPad;
    const int j0 = blockIdx.x * kSlice;
    const int kc_per = R / 8;
    for (int ch = tid; ch < 4 * kSlice * kc_per; ch += kThreads) {
        const int nl = ch / kc_per, kc = ch % kc_per;
        const int col = (nl >> 5) * C + j0 + (nl & 31);
        store_h8(Ws + nl * pitch + 8 * kc, load_h8(P.wrT + (size_t)col * R + 8 * kc));
    }
    __syncthreads();
    const int h = w & 1, l15 = lane & 15, g8 = 8 * (lane >> 4);
    const int j = j0 + 16 * h + l15;
    const float w_ic = h2f(P.peep[j]), w_fc = h2f(P.peep[C + j]), w_oc = h2f(P.peep[2 * C + j]);
    for (int i = 0; i < kTilesPerWg / 2; ++i) {
        const int q0 = (blockIdx.y * kTilesPerWg + (w >> 1) + 2 * i) * 16;
        if (q0 >= n) break;
        const int rowa = q0 + l15 < n ? P.table[off + q0 + l15] : -1;
        const h16 *arow = P.rs + (size_t)max(rowa, 0) * R + g8;
        float4v acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = float4v{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < R / 32; ++s) {
            half8 a = {0, 0, 0, 0, 0, 0, 0, 0};
            if (rowa >= 0) a = load_h8(arow + 32 * s);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const half8 b = load_h8(Ws + (g * kSlice + 16 * h + l15) * pitch + 32 * s + g8);
                acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[g], 0, 0, 0);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = q0 + 4 * (lane >> 4) + k;
            if (q >= n) continue;
            const int row = P.table[off + q];
            const h16 *Gr = P.G + (size_t)row * 4 * C + j;
            const float cp = (P.rinfo[row] & kHasPrev) ? P.c[(size_t)(row - P.ad) * C + j] : 0.f;
            const float ig = sigmoidf(acc[0][k] + h2f(Gr[0]) + w_ic * cp);
            const float fg = sigmoidf(acc[1][k] + h2f(Gr[C]) + w_fc * cp);
            const float gg = tanhf(acc[2][k] + h2f(Gr[2 * C]));
            const float ct = fg * cp + ig * gg;
            const float og = sigmoidf(acc[3][k] + h2f(Gr[3 * C]) + w_oc * ct);
            P.c[(size_t)row * C + j] = ct;
            P.m[(size_t)row * C + j] = f2h(og * tanhf(ct));
            h16 *ga = P.gates + (size_t)row * 4 * C + j;
            ga[0] = f2h(ig);
            ga[C] = f2h(fg);
            ga[2 * C] = f2h(gg);
            ga[3 * C] = f2h(og);
        }
    }
}

// One 16 x 16 tile of A . B^T per workgroup, both operands k-contiguous, the K / 32 steps dealt
// round-robin to the four waves and their accumulators summed through LDS in wave order. arow: the
// lane's A row (row lane & 15 of the tile) or NULL for a row past the end; brow: the lane's B row.
// Returns element (4 (lane >> 4) + w, lane & 15) of the tile: wave w finishes accumulator register w.
__device__ __forceinline__ float lstmp_tile(const h16 *arow, const h16 *brow, int K, int w, int lane) {
    __shared__ float red[4][4][64];
    const int g8 = 8 * (lane >> 4);
    float4v acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = w; s < K / 32; s += 4) {
        half8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (arow) a = load_h8(arow + 32 * s + g8);
        const half8 b = load_h8(brow + 32 * s + g8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[w][k][lane] = acc[k];
    __syncthreads();
    return ((red[0][w][lane] + red[1][w][lane]) + red[2][w][lane]) + red[3][w][lane];
}

// y = W_p m + b_p for a step's rows; r = y[0:R] also into rs at the frame that reads it.
// grid ((R+N) / 16, ceil(n / 16)).
__global__ __launch_bounds__(kThreads) void k_lstmp_proj(LstmpDev P, int off, int n, h16 *y, long long ldy) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15;
    const int n0 = blockIdx.x * 16, q0 = blockIdx.y * 16;
    const int rowa = q0 + l15 < n ? P.table[off + q0 + l15] : -1;
    const float v = lstmp_tile(rowa >= 0 ? P.m + (size_t)rowa * P.C : nullptr, P.wpT + (size_t)(n0 + l15) * P.C, P.C, w, lane);
    const int q = q0 + 4 * (lane >> 4) + w;
    if (q >= n) return;
    const int row = P.table[off + q], col = n0 + l15;
    const h16 hv = f2h(v + h2f(P.bp[col]));
    y[(size_t)row * ldy + col] = hv;
    if (col < P.R && (P.rinfo[row] & kHasNext)) P.rs[(size_t)(row + P.ad) * P.R + col] = hv;
}

// dm = (dy + clip(dr)) W_p^T for a step's rows. grid (C / 16, ceil(n / 16)).
// Prologue (16 threads per row): the row's dr norm, then the fp16 row dy + scale dr into LDS
// As[16][R+N+8]; the workgroups of column tile 0 also store it to dyr for dW_p and db_p.
__global__ __launch_bounds__(kThreads) void k_lstmp_dm(LstmpDev P, int off, int n, const h16 *dy, long long ldy) {
    h16 *As = (h16 *)lstmp_lds;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15;
    const int R = P.R, RN = P.R + P.N, pitch = RN + kPad;
    const int n0 = blockIdx.x * 16, q0 = blockIdx.y * 16;
    {
        const int rl = tid >> 4;
        const int row = q0 + rl < n ? P.table[off + q0 + rl] : -1;
        const bool nxt = row >= 0 && (P.rinfo[row] & kHasNext);
        const float *drr = P.dr + (size_t)max(row, 0) * R;
        float ss = 0.f;
        if (nxt)
            for (int c = l15; c < R; c += 16) ss = fmaf(drr[c], drr[c], ss);
        for (int o = 8; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 16);
        const float nrm = sqrtf(ss);
        const float sc = (P.clip > 0.f && nrm > P.clip) ? P.clip / nrm : 1.f;
        for (int c = l15; c < RN; c += 16) {
            float v = 0.f;
            if (row >= 0) v = h2f(dy[(size_t)row * ldy + c]);
            if (nxt && c < R) v += sc * drr[c];
            const h16 hv = f2h(v);
            As[rl * pitch + c] = hv;
            if (blockIdx.x == 0 && row >= 0) P.dyr[(size_t)row * RN + c] = hv;
        }
    }
    __syncthreads();
    const float v = lstmp_tile(As + l15 * pitch, P.wp + (size_t)(n0 + l15) * RN, RN, w, lane);
    const int q = q0 + 4 * (lane >> 4) + w;
    if (q < n) P.dm[(size_t)q * P.C + n0 + l15] = v;
}

// The nonlinearity's derivative for a step's rows. grid (C / 32, ceil(n / 8)): 8 rows x 32 cells.
// Prologue (32 threads per row): the norm of the row's dc carry over all C cells.
__global__ __launch_bounds__(kThreads) void k_lstmp_step_bwd(LstmpDev P, int off, int n) {
    const int tid = threadIdx.x, rl = tid >> 5, cl = tid & 31;
    const int C = P.C, q = blockIdx.y * 8 + rl;
    const int row = q < n ? P.table[off + q] : -1;
    const int info = row >= 0 ? P.rinfo[row] : 0;
    const float *dcr = P.dc + (size_t)max(row, 0) * C;
    float ss = 0.f;
    if (info & kHasNext)
        for (int c = cl; c < C; c += 32) ss = fmaf(dcr[c], dcr[c], ss);
    for (int o = 16; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 32);
    if (row < 0) return;
    const int j = blockIdx.x * kSlice + cl;
    const float nrm = sqrtf(ss);
    const float sc = (P.clip > 0.f && nrm > P.clip) ? P.clip / nrm : 1.f;
    const float dcar = (info & kHasNext) ? sc * dcr[j] : 0.f;
    const h16 *ga = P.gates + (size_t)row * 4 * C + j;
    const float ig = h2f(ga[0]), fg = h2f(ga[C]), gg = h2f(ga[2 * C]), og = h2f(ga[3 * C]);
    const float ct = P.c[(size_t)row * C + j];
    const float cp = (info & kHasPrev) ? P.c[(size_t)(row - P.ad) * C + j] : 0.f;
    const float w_ic = h2f(P.peep[j]), w_fc = h2f(P.peep[C + j]), w_oc = h2f(P.peep[2 * C + j]);
    const float th = tanhf(ct);
    const float dmv = P.dm[(size_t)q * C + j];
    const float dop = dmv * th * og * (1.f - og);
    const float dct = dcar + dmv * og * (1.f - th * th) + dop * w_oc;
    const float dip = dct * gg * ig * (1.f - ig);
    const float dfp = dct * cp * fg * (1.f - fg);
    const float dgp = dct * ig * (1.f - gg * gg);
    h16 *dg = P.dG + (size_t)row * 4 * C + j;
    dg[0] = f2h(dip);
    dg[C] = f2h(dfp);
    dg[2 * C] = f2h(dgp);
    dg[3 * C] = f2h(dop);
    if (info & kHasPrev) P.dc[(size_t)(row - P.ad) * C + j] = dct * fg + dip * w_ic + dfp * w_fc;
}

// dr[t + d] = dG_t W_r^T for a step's rows. grid (R / 16, ceil(n / 16)).
__global__ __launch_bounds__(kThreads) void k_lstmp_dr(LstmpDev P, int off, int n) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15;
    const int n0 = blockIdx.x * 16, q0 = blockIdx.y * 16, C4 = 4 * P.C;
    const int rowa = q0 + l15 < n ? P.table[off + q0 + l15] : -1;
    const float v = lstmp_tile(rowa >= 0 ? P.dG + (size_t)rowa * C4 : nullptr, P.wr + (size_t)(n0 + l15) * C4, C4, w, lane);
    const int q = q0 + 4 * (lane >> 4) + w;
    if (q >= n) return;
    const int row = P.table[off + q];
    if (P.rinfo[row] & kHasPrev) P.dr[(size_t)(row - P.ad) * P.R + n0 + l15] = v;
}

// Peephole gradients: dw_ic = sum dG_i c', dw_fc = sum dG_f c', dw_oc = sum dG_o c over all rows, in
// double. grid (C / 64, nchunk): 64 columns x 4 row lanes, a chunk's rows dealt round-robin to the
// lanes, the lanes summed in order; k_lstmp_peep_finish sums the chunks in order into the gradient.
__global__ __launch_bounds__(kThreads) void k_lstmp_peep_part(LstmpDev P, int rows, int nchunk) {
    __shared__ double red[3][4][64];
    const int col = threadIdx.x & 63, rlane = threadIdx.x >> 6;
    const int C = P.C, j = blockIdx.x * 64 + col;
    const int per = (rows + nchunk - 1) / nchunk;
    const int r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
    double s[3] = {0.0, 0.0, 0.0};
    if (j < C)
        for (int r = r0 + rlane; r < r1; r += 4) {
            const h16 *dg = P.dG + (size_t)r * 4 * C + j;
            const double cp = (P.rinfo[r] & kHasPrev) ? (double)P.c[(size_t)(r - P.ad) * C + j] : 0.0;
            s[0] = fma((double)h2f(dg[0]), cp, s[0]);
            s[1] = fma((double)h2f(dg[C]), cp, s[1]);
            s[2] = fma((double)h2f(dg[3 * C]), (double)P.c[(size_t)r * C + j], s[2]);
        }
    for (int k = 0; k < 3; ++k) red[k][rlane][col] = s[k];
    __syncthreads();
    if (rlane == 0 && j < C)
        for (int k = 0; k < 3; ++k)
            P.part[((size_t)blockIdx.y * 3 + k) * C + j] = ((red[k][0][col] + red[k][1][col]) + red[k][2][col]) + red[k][3][col];
}
__global__ __launch_bounds__(kThreads) void k_lstmp_peep_finish(LstmpDev P, int nchunk, float *grad) {
    const int i = blockIdx.x * kThreads + threadIdx.x;  // k * C + j
    if (i >= 3 * P.C) return;
    double s = 0.0;
    for (int p = 0; p < nchunk; ++p) s += P.part[(size_t)p * 3 * P.C + i];
    grad[i] += (float)s;
}

KfOperand op_plain(const void *p, long long ld, int rows, int cols, int kcontig) {
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
    d.hout = d.hsrc = d.hdiv = 1;
    d.tpolicy = KF_ZERO;
    for (int i = 0; i < KF_MAX_PARTS; ++i) d.edge_t[i] = -1;
    return d;
}
}  // namespace

struct KfLstmp {
    LstmpDev P{};
    int max_rows = 0, max_seqs = 0;
    float *w32 = nullptr;
    std::vector<void *> blocks;  // every device allocation
    int *lay_dev = nullptr, *lay_pin = nullptr;
    int *table = nullptr, *rinfo = nullptr;
    std::vector<int> lay;        // the layout on the device: seq_row0[B+1], step_off[nsteps+1]
    int B = 0, rows = 0, nsteps = 0;
    const void *x = nullptr;     // the last forward's input
    long long ldx = 0;
    bool has_params = false, has_fwd = false;
    size_t lds_fwd = 0, lds_dm = 0;
};

namespace {
template <typename T>
bool dev_alloc(KfLstmp *l, T *&p, size_t count) {
    void *v = nullptr;
    if (hipMalloc(&v, std::max<size_t>(count * sizeof(T), 16)) != hipSuccess) {
        (void)hipGetLastError();
        lstmp_set_error("kf_lstmp_create: device allocation of %zu bytes failed", count * sizeof(T));
        return false;
    }
    l->blocks.push_back(v);
    p = (T *)v;
    return true;
}

bool launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return true;
    lstmp_set_error("%s: %s", what, hipGetErrorString(e));
    return false;
}

bool hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    (void)hipGetLastError();
    lstmp_set_error("%s: %s", what, hipGetErrorString(e));
    return false;
}

bool gemm_ok(int rc, const char *what) {
    if (rc == 0) return true;
    const char *m = kf_last_error();
    lstmp_set_error("%s: %s", what, m ? m : "failed");
    return false;
}
}  // namespace

extern "C" const char *kf_lstmp_last_error(void) { return lstmp_err_.get(); }

extern "C" void kf_lstmp_free(KfLstmp *l) {
    if (!l) return;
    for (void *p : l->blocks) hipFree(p);
    if (l->lay_pin) hipHostFree(l->lay_pin);
    delete l;
}

extern "C" KfLstmp *kf_lstmp_create(int D, int C, int R, int N, int delay, int max_rows, int max_seqs) {
    lstmp_err_.clear();
    kf_take_pending(__func__);
    if (C <= 0 || C % 32 || R % 32 || N % 32 || R < 0 || N < 0) {
        lstmp_set_error("kf_lstmp_create: C, R and N must be multiples of 32 (C=%d R=%d N=%d)", C, R, N);
        return nullptr;
    }
    if (R == 0) {
        lstmp_set_error("kf_lstmp_create: R = 0: the recurrent projection is what the recurrence reads");
        return nullptr;
    }
    if (delay >= 0) {
        lstmp_set_error("kf_lstmp_create: delay must be negative (delay=%d)", delay);
        return nullptr;
    }
    if (D <= 0 || D % 8) {
        lstmp_set_error("kf_lstmp_create: D must be a multiple of 8 (D=%d)", D);
        return nullptr;
    }
    if (max_rows < 1 || max_seqs < 1) {
        lstmp_set_error("kf_lstmp_create: max_rows and max_seqs must be at least 1 (max_rows=%d max_seqs=%d)", max_rows, max_seqs);
        return nullptr;
    }
    KfLstmp *l = new KfLstmp;
    LstmpDev &P = l->P;
    const long long C4 = 4LL * C, RN = R + N;
    P.D = D, P.C = C, P.R = R, P.N = N, P.ad = -delay;
    P.oB = D * C4;
    P.oWr = P.oB + C4;
    P.oPeep = P.oWr + R * C4;
    P.oWp = P.oPeep + 3 * C;
    P.oBp = P.oWp + C * RN;
    P.total = P.oBp + RN;
    P.clip = 30.f;
    l->max_rows = max_rows, l->max_seqs = max_seqs;
    l->lds_fwd = (size_t)4 * kSlice * (R + kPad) * sizeof(h16);
    l->lds_dm = (size_t)16 * (RN + kPad) * sizeof(h16);
    if (l->lds_fwd > (size_t)kLdsMax || l->lds_dm > (size_t)kLdsMax) {
        lstmp_set_error("kf_lstmp_create: R=%d, N=%d need %zu bytes of LDS per workgroup (at most %d)", R, N,
                        std::max(l->lds_fwd, l->lds_dm), kLdsMax);
        delete l;
        return nullptr;
    }
    const size_t rows = (size_t)max_rows;
    const size_t step_rows = (size_t)std::min<long long>((long long)max_seqs * P.ad, max_rows);
    const size_t nlay = (size_t)max_seqs + 1 + rows + 2;
    bool ok = dev_alloc(l, l->w32, P.total) && dev_alloc(l, P.wx, D * C4) && dev_alloc(l, P.b, C4) &&
              dev_alloc(l, P.wr, R * C4) && dev_alloc(l, P.wrT, R * C4) && dev_alloc(l, P.peep, 3 * C) &&
              dev_alloc(l, P.wp, C * RN) && dev_alloc(l, P.wpT, C * RN) && dev_alloc(l, P.bp, RN) &&
              dev_alloc(l, P.G, rows * C4) && dev_alloc(l, P.gates, rows * C4) && dev_alloc(l, P.c, rows * C) &&
              dev_alloc(l, P.m, rows * C) && dev_alloc(l, P.rs, rows * R) && dev_alloc(l, P.dG, rows * C4) &&
              dev_alloc(l, P.dyr, rows * RN) && dev_alloc(l, P.dr, rows * R) && dev_alloc(l, P.dc, rows * C) &&
              dev_alloc(l, P.dm, step_rows * C) && dev_alloc(l, P.part, (size_t)kPeepChunks * 3 * C) &&
              dev_alloc(l, l->table, rows) && dev_alloc(l, l->rinfo, rows) && dev_alloc(l, l->lay_dev, nlay);
    if (ok && hipHostMalloc((void **)&l->lay_pin, nlay * sizeof(int), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        lstmp_set_error("kf_lstmp_create: pinned allocation of %zu bytes failed", nlay * sizeof(int));
        ok = false;
    }
    if (ok && l->lds_fwd > 48 * 1024 &&
        hipFuncSetAttribute((const void *)k_lstmp_step_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l->lds_fwd) != hipSuccess) {
        (void)hipGetLastError();
        lstmp_set_error("kf_lstmp_create: %zu bytes of LDS refused", l->lds_fwd);
        ok = false;
    }
    if (ok && l->lds_dm > 48 * 1024 &&
        hipFuncSetAttribute((const void *)k_lstmp_dm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l->lds_dm) != hipSuccess) {
        (void)hipGetLastError();
        lstmp_set_error("kf_lstmp_create: %zu bytes of LDS refused", l->lds_dm);
        ok = false;
    }
    if (!ok) {
        kf_lstmp_free(l);
        return nullptr;
    }
    P.table = l->table, P.rinfo = l->rinfo;
    return l;
}

extern "C" long long kf_lstmp_num_params(const KfLstmp *l) { return l ? l->P.total : 0; }

extern "C" int kf_lstmp_set_params(KfLstmp *l, const float *params) {
    kf_take_pending(__func__);
    if (!l || !params) {
        lstmp_set_error("kf_lstmp_set_params: null argument");
        return -1;
    }
    // the working copies may be in use by launches in flight
    if (!hip_ok(hipStreamSynchronize(kf_stream()), "kf_lstmp_set_params") ||
        !hip_ok(hipMemcpy(l->w32, params, l->P.total * sizeof(float), hipMemcpyHostToDevice), "kf_lstmp_set_params"))
        return -1;
    kf_launch(k_lstmp_cast, dim3(kf_blocks(l->P.total, kThreads)), dim3(kThreads), 0, nullptr, l->P, l->w32);
    if (!launched("kf_lstmp_set_params")) return -1;
    l->has_params = true;
    return 0;
}

extern "C" int kf_lstmp_get_params(const KfLstmp *l, float *params) {
    kf_take_pending(__func__);
    if (!l || !params) {
        lstmp_set_error("kf_lstmp_get_params: null argument");
        return -1;
    }
    return hip_ok(hipMemcpy(params, l->w32, l->P.total * sizeof(float), hipMemcpyDeviceToHost), "kf_lstmp_get_params") ? 0 : -1;
}

extern "C" int kf_lstmp_set_clip(KfLstmp *l, float threshold) {
    if (!l || !(threshold >= 0.f)) {
        lstmp_set_error("kf_lstmp_set_clip: the threshold must be >= 0 (0 = off)");
        return -1;
    }
    l->P.clip = threshold;
    return 0;
}

extern "C" int kf_lstmp_state(const KfLstmp *l, const float **c, const void **m, const void **gates) {
    if (!l || !l->has_fwd) {
        lstmp_set_error("kf_lstmp_state: no forward yet");
        return -1;
    }
    if (c) *c = l->P.c;
    if (m) *m = l->P.m;
    if (gates) *gates = l->P.gates;
    return 0;
}

extern "C" int kf_lstmp_forward(KfLstmp *l, const void *x_dev, long long ldx, const int32_t *seq_row0, int B,
                                void *y_dev, long long ldy) {
    kf_take_pending(__func__);
    if (!l || !x_dev || !seq_row0 || !y_dev) {
        lstmp_set_error("kf_lstmp_forward: null argument");
        return -1;
    }
    const LstmpDev &P = l->P;
    const int C4 = 4 * P.C, RN = P.R + P.N, ad = P.ad;
    if (!l->has_params) {
        lstmp_set_error("kf_lstmp_forward: no parameters set");
        return -1;
    }
    if (B < 1 || B > l->max_seqs) {
        lstmp_set_error("kf_lstmp_forward: %d sequences, the operator was created for 1 .. %d (max_seqs)", B, l->max_seqs);
        return -1;
    }
    if (seq_row0[0] != 0) {
        lstmp_set_error("kf_lstmp_forward: seq_row0[0] must be 0");
        return -1;
    }
    int maxlen = 0;
    for (int i = 0; i < B; ++i) {
        if (seq_row0[i + 1] < seq_row0[i]) {
            lstmp_set_error("kf_lstmp_forward: seq_row0 decreases at sequence %d", i);
            return -1;
        }
        maxlen = std::max(maxlen, seq_row0[i + 1] - seq_row0[i]);
    }
    const int rows = seq_row0[B];
    if (rows > l->max_rows || rows < 1) {
        lstmp_set_error("kf_lstmp_forward: %d rows, the operator was created for 1 .. %d (max_rows)", rows, l->max_rows);
        return -1;
    }
    if (ldx < P.D || ldx % 8 || ((uintptr_t)x_dev & 15) || ldy < RN) {
        lstmp_set_error("kf_lstmp_forward: ldx >= D, ldx %% 8 == 0, x 16-byte aligned and ldy >= R + N required (ldx=%lld ldy=%lld)",
                        ldx, ldy);
        return -1;
    }
    // the layout: seq_row0, then the steps' offsets into the row table
    const int nsteps = (maxlen + ad - 1) / ad;
    std::vector<int> lay((size_t)B + 1 + nsteps + 1);
    for (int i = 0; i <= B; ++i) lay[i] = seq_row0[i];
    int *so = lay.data() + B + 1;
    so[0] = 0;
    for (int s = 0; s < nsteps; ++s) {
        int n = 0;
        for (int i = 0; i < B; ++i) n += std::min(std::max(seq_row0[i + 1] - seq_row0[i] - s * ad, 0), ad);
        so[s + 1] = so[s] + n;
    }
    hipStream_t st = kf_stream();
    l->has_fwd = false;
    if (lay != l->lay || B != l->B) {
        // the pinned staging may still be the source of the previous upload
        l->lay.clear();
        if (!hip_ok(hipStreamSynchronize(st), "kf_lstmp_forward")) return -1;
        memcpy(l->lay_pin, lay.data(), lay.size() * sizeof(int));
        if (!hip_ok(hipMemcpyAsync(l->lay_dev, l->lay_pin, lay.size() * sizeof(int), hipMemcpyHostToDevice, st),
                    "kf_lstmp_forward"))
            return -1;
    }
    const int prof = kf_prof_start(KF_PROF_LSTMP_FWD, 2.0 * rows * ((double)C4 * (P.D + P.R) + (double)P.C * RN));
    kf_launch(k_lstmp_prep, dim3(B + 1), dim3(kThreads), 0, nullptr, (const int *)l->lay_dev, B, nsteps, ad, P.R, l->table,
              l->rinfo, P.rs);
    KfOperand A = op_plain(x_dev, ldx, rows, P.D, 1);
    KfOperand Bw = op_plain(P.wx, C4, P.D, C4, 0);
    KfEpilogue E;
    memset(&E, 0, sizeof E);
    E.alpha = 1.f;
    E.out = P.G;
    E.ldo = C4;
    E.bias = P.b;
    if (!gemm_ok(kf_gemm_fused(rows, C4, P.D, &A, &Bw, &E), "kf_lstmp_forward: G = X W_x + b")) return -1;
    for (int s = 0; s < nsteps; ++s) {
        const int off = so[s], n = so[s + 1] - so[s];
        kf_launch(k_lstmp_step_fwd, dim3(P.C / kSlice, (n + 16 * kTilesPerWg - 1) / (16 * kTilesPerWg)), dim3(kThreads),
                  l->lds_fwd, nullptr, P, off, n);
        kf_launch(k_lstmp_proj, dim3(RN / 16, (n + 15) / 16), dim3(kThreads), 0, nullptr, P, off, n, (h16 *)y_dev, ldy);
    }
    kf_prof_stop(prof);
    if (!launched("kf_lstmp_forward")) return -1;
    l->lay.swap(lay);
    l->B = B, l->rows = rows, l->nsteps = nsteps;
    l->x = x_dev, l->ldx = ldx;
    l->has_fwd = true;
    return 0;
}

extern "C" int kf_lstmp_backward(KfLstmp *l, const void *dy_dev, long long ldy, void *dx_dev, long long ldx,
                                 float *grad_dev) {
    kf_take_pending(__func__);
    if (!l || !dy_dev || !grad_dev) {
        lstmp_set_error("kf_lstmp_backward: null argument");
        return -1;
    }
    if (!l->has_fwd) {
        lstmp_set_error("kf_lstmp_backward: no forward before it");
        return -1;
    }
    const LstmpDev &P = l->P;
    const int C4 = 4 * P.C, RN = P.R + P.N, rows = l->rows;
    if (ldy < RN || (dx_dev && (ldx < P.D || ldx % 8 || ((uintptr_t)dx_dev & 15)))) {
        lstmp_set_error("kf_lstmp_backward: ldy >= R + N, ldx >= D, ldx %% 8 == 0 and dx 16-byte aligned required (ldy=%lld ldx=%lld)",
                        ldy, ldx);
        return -1;
    }
    const int *so = l->lay.data() + l->B + 1;
    const int prof = kf_prof_start(KF_PROF_LSTMP_BWD, 4.0 * rows * ((double)C4 * (P.D + P.R) + (double)P.C * RN));
    for (int s = l->nsteps - 1; s >= 0; --s) {
        const int off = so[s], n = so[s + 1] - so[s];
        kf_launch(k_lstmp_dm, dim3(P.C / 16, (n + 15) / 16), dim3(kThreads), l->lds_dm, nullptr, P, off, n,
                  (const h16 *)dy_dev, ldy);
        kf_launch(k_lstmp_step_bwd, dim3(P.C / kSlice, (n + 7) / 8), dim3(kThreads), 0, nullptr, P, off, n);
        if (s > 0) kf_launch(k_lstmp_dr, dim3(P.R / 16, (n + 15) / 16), dim3(kThreads), 0, nullptr, P, off, n);
    }
    if (!launched("kf_lstmp_backward")) return -1;
    // the products over all rows
    KfOperand dG = op_plain(P.dG, C4, rows, C4, 0);
    KfOperand X = op_plain(l->x, l->ldx, rows, P.D, 0);
    KfOperand Rs = op_plain(P.rs, P.R, rows, P.R, 0);
    KfOperand M = op_plain(P.m, P.C, rows, P.C, 0);
    KfOperand Dyr = op_plain(P.dyr, RN, rows, RN, 0);
    if (!gemm_ok(kf_gemm_wgrad(P.D, C4, rows, &X, &dG, grad_dev, C4, grad_dev + P.oB, 1), "kf_lstmp_backward: dW_x") ||
        !gemm_ok(kf_gemm_wgrad(P.R, C4, rows, &Rs, &dG, grad_dev + P.oWr, C4, nullptr, 1), "kf_lstmp_backward: dW_r") ||
        !gemm_ok(kf_gemm_wgrad(P.C, RN, rows, &M, &Dyr, grad_dev + P.oWp, RN, grad_dev + P.oBp, 1), "kf_lstmp_backward: dW_p"))
        return -1;
    if (dx_dev) {
        KfOperand A = op_plain(P.dG, C4, rows, C4, 1);
        KfOperand Bw = op_plain(P.wx, C4, P.D, C4, 1);
        KfEpilogue E;
        memset(&E, 0, sizeof E);
        E.alpha = 1.f;
        E.out = dx_dev;
        E.ldo = ldx;
        if (!gemm_ok(kf_gemm_fused(rows, P.D, C4, &A, &Bw, &E), "kf_lstmp_backward: dX")) return -1;
    }
    const int nchunk = std::min(kPeepChunks, (rows + 63) / 64);
    kf_launch(k_lstmp_peep_part, dim3((P.C + 63) / 64, nchunk), dim3(kThreads), 0, nullptr, P, rows, nchunk);
    kf_launch(k_lstmp_peep_finish, dim3(kf_blocks(3 * P.C, kThreads)), dim3(kThreads), 0, nullptr, P, nchunk,
              grad_dev + P.oPeep);
    kf_prof_stop(prof);
    return launched("kf_lstmp_backward") ? 0 : -1;
}
