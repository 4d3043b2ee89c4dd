// chain_denom.h — the denominator unit's interface (chain_den.hip) to the reference ABI
// (chain_abi.hip) and the product interface (chain.hip): the SELL-64 table and run
// structs its kernels take, the exchange descriptor and its buffers, the device tables of
// a graph, and the host launch entries. The kernels themselves are defined, instantiated
// and launched in chain_den.hip alone.
#pragma once
#include "chain_dev.h"
#include "chain_tables.h"
#include "../../include/kf_chain.h"

// ===========================================================================
// Denominator (prob space, leaky HMM) — SELL-64 arc tables
// ===========================================================================
struct SellDev {  // sliced ELL, 64 rows per slice, rows sorted by degree
    int nsl;
    const int *perm, *len, *off;
    // records {f1 | f2 << 16, tp} with f1, f2 as the LDS byte offsets of their operands
    // in rows interleaving NS sequences (f, b) or frames (q): 4 * NS * f1, 4 * NS * f2,
    // index NS - 1 — one address add per gather
    const uint2 *arc_p[2];
    const float *initp;   // init[perm[c]] in slice order (0 for padding rows), f and b only
    // Slice ownership for G = 1, 2, 4, 8 blocks per sequence (index log2 G): the slices
    // are spread over the G x DEN_WAVES (block, wave) pairs by length, longest first onto
    // the least loaded pair, so the slowest wave of a frame carries about the mean share
    // (round-robin ownership left it 1.3-1.4x the mean on the den graph's degree-sorted
    // slices). slot[lgG][gi * spg + k]: the slice in slot k of block gi, processed by
    // wave k % DEN_WAVES (-1: empty). The q table keeps only its G = 1 lists (the
    // posterior kernel's waves).
    const int *slot[4];
    int spg[4];
};
struct DenDev {
    int S, P;
    SellDev f;  // rows = destination states: {src, pdf0}
    SellDev b;  // rows = source states:      {dst, pdf0}
    SellDev q;  // rows = pdfs:               {src, dst}
    const float *init;
    int pair_ok;  // the NS = 2 recursion fits the LDS
};

struct DenRun {
    const void *nnet;
    long long ld;
    const long long *row0;  // [nseq]
    const int *frames;      // [nseq]
    int stride, max_frames;
    float leaky;
    int backward;           // 0: forward only
    float *den_out;         // [nseq][2] {total_prob, log-prob} from k_den_fwd
    unsigned long long *trace;  // optional phase timestamps (kf_chain_trace), null = off
    float *alpha_store;     // [nseq][max_frames+1][nsl_f*64], forward-table slice order
    float *beta_store;      // [nseq][max_frames+1][nsl_b*64], backward-table slice order
    float *asum_store;      // [nseq][max_frames+1] alpha sums (alpha'[t] = row + asum[t]*leaky*init)
    float *bsum_store;      // [nseq][max_frames+1] <init, beta'[t]> (beta[t] = row + leaky*bsum[t])
    float *stats;           // [nseq][8]
    // ABI mode
    float *post_dense;      // [T x P] (single sequence)
    // product mode
    const LogFstDev *nums;  // [nseq] numerator descriptors (total, G, grp_pdf, post_sparse)
    h16 *out_grad;
    long long ldg;
    KfChainOpts opts;
    // kf_chain_compute_weighted, null = ones
    const float *seq_w;     // [nseq] the example's weight (times opts.supervision_weight)
    const float *frame_w;   // [nseq][max_frames] deriv weight of (sequence, frame)
    // kf_chain_set_grad_scale, null = 1: one device float, the factor on the finished
    // derivative row before its one rounding to fp16
    const float *grad_scale;
};

enum { DEN_ABI = 0, DEN_PRODUCT = 1 };

// NS = 2: the blocks of a unit run two sequences at once. The LDS state is
// interleaved (float2 per state), so one SELL record, one pair of address adds and
// two 8-byte gathers serve both sequences (the record stream and the gather issue of
// the arc phase halve per sequence); G doubles so the grid keeps every CU busy.
struct DenX {
    float *buf;     // [nseq][2][G][blk]; blk = 64: [q * DEN_WAVES + wave] = that wave's partial
                    // sum of sequence q of the unit (the state slices themselves are exchanged
                    // through the alpha / beta stores)
    unsigned *cnt;  // [nseq] arrivals (zeroed before each launch)
    unsigned *xm;   // [nseq] XCD census: 4-bit arrival count per XCD (zeroed before each launch)
    int force_sys;  // 1: agent-scope exchange even when a unit's blocks share an XCD (tests)
    unsigned *tmo;  // per-launch timeout word (zeroed before each launch)
    unsigned *sticky;  // timed-out blocks since the last read (never zeroed by a launch)
    unsigned spin_limit;  // polls before a wait gives up (kf_chain_debug_spin_limit)
    int G, lgG, spg, blk;  // spg: exchange slots per block (the table's at this G)
    int nseq;              // exchange units (NS sequences each: 2u, 2u+1 for NS = 2)
    int nseqs, ns;         // sequences, sequences per unit
    unsigned lds_f, lds_b; // dynamic LDS of the fwd / bwd kernels
};

#pragma GCC visibility push(hidden)  // internal to libkaldi_fp16.so

struct DenTables {
    DenDev dev{};
    std::vector<void *> owned;
    ~DenTables() {
        for (void *p : owned) hipFree(p);
    }
};

// validates the graph (chain_tables.cpp), builds and uploads its tables; null with *why set
DenTables *make_den_tables(int S, int P, int A, const int32_t *src, const int32_t *dst,
                           const int32_t *pdf0, const float *tp, const char **why);
void den_tables_set_init(const DenDev &d, const float *d_init, hipStream_t st);
int den_pick_G(int nseq);

// exchange buffers + counters for up to nseq sequences at G blocks each
struct DenXBuf {
    float *buf = nullptr;
    unsigned *cnt = nullptr;
    size_t buf_cap = 0, cnt_cap = 0;
    ~DenXBuf() {
        if (buf) hipFree(buf);
        if (cnt) hipFree(cnt);
        if (h_word) hipHostFree(h_word);
    }
    // nseqs sequences in units of ns, G blocks per unit, over table `tb` (the f table for
    // the forward recursion, b for the backward)
    bool make(const DenDev &g, const SellDev &tb, int nseqs, int ns, int G, DenX &X) {
        X.G = G;
        X.ns = ns;
        X.nseqs = nseqs;
        X.nseq = (nseqs + ns - 1) / ns;
        X.lgG = G == 8 ? 3 : G == 4 ? 2 : G == 2 ? 1 : 0;
        X.spg = tb.spg[X.lgG];
        X.blk = 64;  // partial sums only: the slices go through the alpha / beta stores
        X.lds_f = (unsigned)den_rec_fixed_bytes(g.P, g.f.nsl, g.f.spg[X.lgG], ns);
        X.lds_b = (unsigned)den_rec_fixed_bytes(g.P, g.b.nsl, g.b.spg[X.lgG], ns);
        size_t nb = (size_t)X.nseq * 2 * G * X.blk * 4;
        size_t nc = (((size_t)X.nseq * 2 + 2) * 4 + 15) / 16 * 16;  // sticky, timeout, counters, census
        if (nb > buf_cap) {
            if (buf) hipFree(buf);
            buf = nullptr;
            buf_cap = 0;
            if (hipMalloc(&buf, nb) != hipSuccess) return false;
            buf_cap = nb;
        }
        if (nc > cnt_cap) {
            unsigned *grown = nullptr;
            if (hipMalloc(&grown, nc) != hipSuccess) return false;
            hipMemsetAsync(grown, 0, nc, kf_stream());
            if (cnt) {  // the sticky count survives the reallocation
                hipMemcpyAsync(grown, cnt, 4, hipMemcpyDeviceToDevice, kf_stream());
                hipStreamSynchronize(kf_stream());
                hipFree(cnt);
            }
            cnt = grown;
            cnt_cap = nc;
        }
        X.buf = buf;
        X.sticky = cnt;
        X.tmo = cnt + 1;
        X.cnt = cnt + 2;
        X.xm = cnt + 2 + X.nseq;
        X.spin_limit = spin_limit;
        X.force_sys = force_sys;
        last_units = X.nseq;
        last_G = G;
        return true;
    }
    int last_units = 0, last_G = 0;
    // units of the last launch whose G workgroups all ran on one XCD (the census words
    // stay in memory after the launch); -1 on a read error
    int census_local(hipStream_t st) {
        if (!cnt || !last_units) return 0;
        std::vector<unsigned> w(last_units);
        hipMemcpyAsync(w.data(), cnt + 2 + last_units, (size_t)last_units * 4, hipMemcpyDeviceToHost, st);
        if (hipStreamSynchronize(st) != hipSuccess) return -1;
        int n = 0;
        for (unsigned v : w)
            for (int k = 0; k < 8; ++k)
                if (((v >> (4 * k)) & 15) == (unsigned)last_G) {
                    ++n;
                    break;
                }
        return n;
    }
    // counters and the per-launch timeout word; never the sticky word
    void zero(hipStream_t st) { hipMemsetAsync(cnt + 1, 0, cnt_cap - 4, st); }
    unsigned spin_limit = 1u << 21;
    int force_sys = 0;
    // blocks that timed out since the last call (stream-ordered read, then cleared)
    // (read through a pinned word: a stream-ordered copy into pageable memory left
    // hipErrorStreamCaptureUnsupported pending on the calling thread in the r6 bench)
    unsigned *h_word = nullptr;
    unsigned take_timeouts(hipStream_t st) {
        if (!cnt) return 0;
        if (!h_word && hipHostMalloc((void **)&h_word, 64, hipHostMallocDefault) != hipSuccess) {
            h_word = nullptr;
            kf_take_pending("DenXBuf::take_timeouts hipHostMalloc");
            return 0;
        }
        *h_word = 0;
        hipMemcpyAsync(h_word, cnt, 4, hipMemcpyDeviceToHost, st);
        kf_take_pending("DenXBuf::take_timeouts hipMemcpyAsync");
        hipStreamSynchronize(st);
        kf_take_pending("DenXBuf::take_timeouts hipStreamSynchronize");
        const unsigned v = *h_word;
        if (v) {
            hipMemsetAsync(cnt, 0, 4, st);
            hipStreamSynchronize(st);
        }
        return v;
    }
};

// the launches, on kf_stream(); fp32_in: the den ABI's fp32 rows (one sequence)
void launch_den_fwd(const DenDev &g, const DenRun &r, const DenX &X, DenXBuf &xb, bool fp32_in);
void launch_den_fb(const DenDev &g, const DenRun &r, const DenX &XF, DenXBuf &xf, const DenX &XB,
                   DenXBuf &xbb, bool fp32_in);
void launch_den_post(const DenDev &g, const DenRun &r, const DenX &X, bool fp32_in, int mode);

#pragma GCC visibility pop
