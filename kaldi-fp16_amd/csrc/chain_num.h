// chain_num.h — the numerator unit's interface (chain_num.hip) to the reference ABI
// (chain_abi.hip) and the product interface (chain.hip): the uploaded FSTs of a batch and
// the host launch entries. The kernels are defined and launched in chain_num.hip alone.
#pragma once
#include "chain_dev.h"
#include "chain_tables.h"
#include "../../include/chain.h"

#pragma GCC visibility push(hidden)  // internal to libkaldi_fp16.so

// Packs many NumHost into one device blob; fills LogFstDev pointer fields.
struct NumDevice {
    std::vector<LogFstDev> desc;  // per FST, pointers set, run fields unset
    std::vector<int> G, Ag;
    std::vector<void *> owned;
    ~NumDevice() {
        for (void *p : owned) hipFree(p);
    }
};

// descriptors of the FSTs packed at device address d
void num_descs(const std::vector<NumHost> &hs, const std::vector<std::vector<size_t>> &offs,
               const int32_t *d, NumDevice *nd);
NumDevice *upload_nums(std::vector<NumHost> &hs, const char **why);
// ABI helper: device ChainFstGPU -> host NumHost
bool fetch_fst(const ChainFstGPU *fst, NumHost &h, const char **why);
// Runs k_logfb over `fsts` (already filled) and returns the totals.
bool run_logfb(std::vector<LogFstDev> &fsts, const void *nnet16, long long ld, int P,
               std::vector<float> &totals, const char **why);

// dynamic LDS of k_num_fb for the batch's first nseq FSTs (descriptors with S, A, G set);
// 0: one of them does not fit, the batch runs k_logfb
size_t num_batch_lds(const std::vector<LogFstDev> &desc, const std::vector<int> &Ag, int nseq);
// the batched numerator on `st`: k_num_fb + k_num_post over device descriptors `fsts` when
// num_lds > 0, else k_logfb; maxT = the longest sequence's frames
void launch_num_batch(const LogFstDev *fsts, const h16 *nnet, long long ld, int P, int nseq, int maxT,
                      size_t num_lds, hipStream_t st);

#pragma GCC visibility pop
