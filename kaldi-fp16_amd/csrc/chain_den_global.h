// chain_den_global.h — the global-rows denominator's interface (chain_den_global.hip) to the
// product interface (chain.hip): the device tables of a graph, the workspace of a KfChain and the
// run struct its kernels take. The kernels are defined and launched in chain_den_global.hip alone.
#pragma once
#include "chain_dev.h"
#include "chain_tables.h"
#include "../../include/kf_chain.h"

#define DG_THREADS 1024
#define DG_WAVES 16
#define DG_MAXWG 256  // workgroups of one recursion or posterior launch (= partial sums per frame)

struct DgTabDev {
    int nrows;            // padded to a multiple of 64
    const int *rowptr;    // [nrows + 1]
    const int *perm;      // [nrows] row -> state / pdf, -1 for padding rows
    const uint2 *rec;     // {f1 | f2 << 16, tp}, rows contiguous, arc order
    const float *ti;      // tp * init[src] per record (f and q tables: the leaky term of alpha')
    const float *initp;   // init[perm[r]] per row, 0 for padding (f and b tables)
};
struct DgDev {
    int S, P, A;
    DgTabDev f, b, q;
    float as0;  // sum(init), summed in state order on the host
};

// Workspace of a KfChain for `slots` = groups x NQ sequence slots and max_frames (mf) frames. Every
// row interleaves the NQ sequences of a group, q fastest; a group's share of an array is slots-
// proportional, so one allocation serves every NQ <= the one it was sized for.
struct DgWork {
    float *alpha;  // [grp][mf + 1][RS][NQ]  alpha[t] before the leaky term, f-table row order
    float *beta;   // [grp][mf][RS][NQ]      beta'[t], t = 1 .. T - 1, b-table row order
    float *e;      // [grp][mf][P][NQ]       exp(clamp(x)), then the frame's posteriors in place
    float *apart;  // [grp][mf + 1][DG_MAXWG][NQ] per-workgroup partials of sum(alpha[t])
    float *bpart;  // [grp][mf + 1][DG_MAXWG][NQ] ... of <init, beta'[t]>
    float *gpart;  // [grp][mf][DG_MAXWG][NQ]     ... of the frame's posterior sum
    float *asum;   // [grp][mf + 1][NQ] the partials summed (k_dg_sums)
    float *bsum;   // [grp][mf + 1][NQ]
    float *fpart;  // [slots][mf][2] {out-of-range count, sum x^2} of a (sequence, frame)
};

struct DgRun {
    const void *nnet;
    long long ld;
    const long long *row0;  // [nseq]
    const int *frames;      // [nseq]
    int stride, max_frames;
    int nseq, NQ, ngrp, Tm;  // sequences, sequences per group (power of two <= 64), groups, longest
    float leaky;
    DgWork w;
    float *den_out;  // [nseq][2] {total_prob, log-prob}
    float *stats;    // [nseq][8]
    const LogFstDev *nums;
    h16 *out_grad;
    long long ldg;
    KfChainOpts opts;
    const float *seq_w, *frame_w, *grad_scale;  // as DenRun's
};

#pragma GCC visibility push(hidden)  // internal to libkaldi_fp16.so

struct DgTables {
    DgDev dev{};
    std::vector<void *> owned;
    ~DgTables() {
        for (void *p : owned) hipFree(p);
    }
};
// validates the graph (chain_tables.cpp), builds and uploads its tables; null with *why set
DgTables *make_dg_tables(int S, int P, int A, const int32_t *src, const int32_t *dst, const int32_t *pdf0,
                         const float *tp, const float *init, const char **why);

inline int dg_pick_nq(int nseq) {
    int nq = 1;
    while (nq < nseq && nq < 64) nq *= 2;
    return nq;
}
inline int dg_slots(int nseq) {
    const int nq = dg_pick_nq(nseq);
    return (nseq + nq - 1) / nq * nq;
}
// bytes of the workspace; *w (optional) gets the arrays' places behind `base`
size_t dg_work_bytes(const DgDev &g, int max_seqs, int max_frames, float *base, DgWork *w);

// the launches, on kf_stream(): staging, both recursions frame by frame, the sums and den_lp;
// then (the numerator's posteriors must be in) the posteriors, the assembly and the statistics
void launch_dg_recursions(const DgDev &g, const DgRun &r);
void launch_dg_post(const DgDev &g, const DgRun &r);

#pragma GCC visibility pop
