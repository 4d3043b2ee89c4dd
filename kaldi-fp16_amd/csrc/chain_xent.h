// chain_xent.h — the xent unit's interface (chain_xent.hip) to the product interface
// (chain.hip): the run of k_chain_xent and its host launch entry. The kernel is defined,
// instantiated and launched in chain_xent.hip alone.
#pragma once
#include "chain_dev.h"

#pragma GCC visibility push(hidden)  // internal to libkaldi_fp16.so

// One kf_chain_xent: the layout is that of the kf_chain_compute before it (device arrays of
// the KfChain), the matrices are the xent output and its gradient.
struct XentRun {
    const LogFstDev *nums;   // [nseq] numerator descriptors: G, grp_pdf, post_sparse [T x G]
    const long long *row0;   // [nseq] frame t of sequence i is row row0[i] + t * stride
    const int *frames;       // [nseq]
    const float *stats;      // [nseq][8], [7] = ok
    const h16 *y;            // fp16 log-softmax rows, leading dimension ldx
    long long ldx;
    h16 *grad;               // fp16 loss gradient at the affine output, leading dimension ldg
    long long ldg;
    float *part;             // [nseq][part_ld] per-frame w * sum_p post[p] y[p]
    int part_ld;
    int max_t;               // frames of the longest sequence: block b is frame b % max_t of sequence b / max_t
    int P, stride;
    float w, scale;          // supervision weight, xent_regularize * w
    // after a kf_chain_compute_weighted, null = ones
    float xr;                // xent_regularize: with seq_w, scale = xr * (w * seq_w[i])
    const float *seq_w;      // [nseq]
    const float *frame_w;    // [nseq][part_ld]
    const float *grad_scale; // kf_chain_set_grad_scale, null = 1: one device float
};

// total_frames = all supervised frames (the profile record's bytes)
void launch_chain_xent(const XentRun &r, int nseq, double total_frames);

#pragma GCC visibility pop
