// chain_xent.hip — the xent output's derivative and objective from the numerator posteriors
// kf_chain_compute left behind (kf_chain.h kf_chain_xent): Kaldi's chain training
// with --chain.xent-regularize. For a supervised row, with post the numerator posteriors as
// a dense row (out-of-range pdfs dropped) and S their computed sum,
//   grad[p] = rne(f (-xr w (post[p] - exp(y[p]) S)))    objf += w post[p] y[p]
// (w = w_i and f the frame's deriv weight after a weighted compute; else f = 1)
// i.e. the posteriors scaled by the supervision weight (Kaldi's xent_output_deriv) taken
// back through the log-softmax (LogSoftmaxComponent::Backprop), as a loss gradient.
// One workgroup per (sequence, frame), as k_den_post's product mode handles the same sparse
// rows: a dense fp32 row in LDS, zero-filled, the G posteriors scattered into it, then one
// dense pass that reads every y once and writes every grad once (exp through the hardware's
// exp2: its error, about 2^-21 relative, is far inside fp16's rounding). No atomics; every sum in a
// fixed order (block_sum), so a call replays bit for bit. Algorithmic traffic: 4 P bytes per row
// (measured at 2.5 x a copy of those bytes).
#include "chain_xent.h"
#include "kf_prof.h"

constexpr int XENT_THREADS = 256, XENT_WAVES = XENT_THREADS / 64;
// columns of the LDS row (8 KiB); a wider output (P <= 4096: two chunks at most) runs in column
// chunks of this many
constexpr int XENT_CHUNK = 2048;
static_assert(XENT_CHUNK == 8 * XENT_THREADS, "k_chain_xent<true>: one 16-byte vector per thread and chunk");

// VEC: P, ldx and ldg are multiples of 8 and both bases 16-byte aligned, so each thread moves
// 8 columns per 16-byte load and store; else one column at a time
template <bool VEC>
__global__ __launch_bounds__(XENT_THREADS) void k_chain_xent(const XentRun r) {
    __shared__ __attribute__((aligned(16))) float row[XENT_CHUNK];
    __shared__ float red_s[XENT_WAVES], red_o[XENT_WAVES];
    const int seq = blockIdx.x / r.max_t, t = blockIdx.x % r.max_t, tid = threadIdx.x;
    if (t >= r.frames[seq]) return;
    const LogFstDev *nf = &r.nums[seq];
    const int G = nf->G, P = r.P;
    const int *gp = nf->grp_pdf;
    const float *nps = nf->post_sparse + (size_t)t * G;
    const long long ri = r.row0[seq] + (long long)t * r.stride;
    h16 *g = r.grad + ri * r.ldg;
    // a sequence whose objective was not finite: zero rows, no objective
    const bool ok = r.stats[(size_t)seq * 8 + 7] > 0.5f;
    if (!ok) {
        if constexpr (VEC) {
            half8 z;
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = (h16)0.0f;
            for (int j = tid * 8; j < P; j += XENT_THREADS * 8) store_h8(g + j, z);
        } else {
            for (int j = tid; j < P; j += XENT_THREADS) g[j] = (h16)0.0f;
        }
        if (tid == 0) r.part[(size_t)seq * r.part_ld + t] = 0.0f;
        return;
    }
    const h16 *y = r.y + ri * r.ldx;
    // VEC: a chunk is one 16-byte vector per thread (XENT_CHUNK = 8 * XENT_THREADS). Chunk 0's
    // vector is requested before anything else and chunk c + 1's at the top of chunk c, so the
    // HBM latency of y runs under the descriptor reads, the sum and the LDS scatter
    half8 ynext;
    if constexpr (VEC) {
        if (tid * 8 < P) ynext = load_h8(y + tid * 8);
    }
    float sp = 0.f;
    for (int q = tid; q < G; q += XENT_THREADS) {
        const int p = gp[q];
        if (p > 0 && p <= P) sp += nps[q];
    }
    const float S = block_sum<XENT_WAVES>(sp, red_s);
    float w = r.w, scale = r.scale;
    if (r.seq_w) {  // the weighted compute's w_i, block-uniform
        w = r.w * r.seq_w[seq];
        scale = r.xr * w;
    }
    // (the loss scale, DESIGN §30: one more block-uniform load beside the frame weight)
    float fw = r.frame_w ? r.frame_w[(size_t)seq * r.part_ld + t] : 1.0f;
    if (r.grad_scale) fw *= *r.grad_scale;
    const bool zero = !(scale != 0.0f);
    float ob = 0.f;
    for (int c0 = 0; c0 < P; c0 += XENT_CHUNK) {
        const int n = min(XENT_CHUNK, P - c0), j8 = tid * 8;
        half8 yv;
        if constexpr (VEC) {
            yv = ynext;
            if (c0 + XENT_CHUNK + j8 < P) ynext = load_h8(y + c0 + XENT_CHUNK + j8);
        }
        for (int j = tid; j < n; j += XENT_THREADS) row[j] = 0.f;
        __syncthreads();
        for (int q = tid; q < G; q += XENT_THREADS) {  // (distinct pdfs: no two writers of a slot)
            const int j = gp[q] - 1 - c0;
            if (j >= 0 && j < n) row[j] = nps[q];
        }
        __syncthreads();
        if constexpr (VEC) {
            if (j8 < n) {
                const float4v p0 = *reinterpret_cast<const float4v *>(row + j8);
                const float4v p1 = *reinterpret_cast<const float4v *>(row + j8 + 4);
                half8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float po = e < 4 ? p0[e & 3] : p1[e & 3], yf = (float)yv[e];
                    if (po != 0.f) ob += po * yf;
                    o[e] = zero ? (h16)0.0f : f2h(fw * (-scale * (po - __expf(yf) * S)));
                }
                store_h8(g + c0 + j8, o);
            }
        } else {
            for (int j = tid; j < n; j += XENT_THREADS) {
                const float po = row[j], yf = (float)y[c0 + j];
                if (po != 0.f) ob += po * yf;
                g[c0 + j] = zero ? (h16)0.0f : f2h(fw * (-scale * (po - __expf(yf) * S)));
            }
        }
        __syncthreads();  // the next chunk's zero fill
    }
    const float o = block_sum<XENT_WAVES>(ob, red_o);
    if (tid == 0) r.part[(size_t)seq * r.part_ld + t] = w * o;
}

void launch_chain_xent(const XentRun &r, int nseq, double total_frames) {
    if (nseq <= 0 || r.max_t <= 0) return;
    // (a block past its sequence's frames returns at once)
    const long long nblk = (long long)nseq * r.max_t;
    const bool vec = r.P % 8 == 0 && r.ldx % 8 == 0 && r.ldg % 8 == 0 && ((uintptr_t)r.y & 15) == 0 &&
                     ((uintptr_t)r.grad & 15) == 0;
    KfProfRec rec{};
    rec.cls = KF_PROF_CHAIN_XENT;
    rec.bytes = total_frames * 4.0 * r.P;
    if (vec) kf_launch(k_chain_xent<true>, dim3((unsigned)nblk), dim3(XENT_THREADS), 0, &rec, r);
    else kf_launch(k_chain_xent<false>, dim3((unsigned)nblk), dim3(XENT_THREADS), 0, &rec, r);
}
