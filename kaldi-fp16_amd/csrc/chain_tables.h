// chain_tables.h — host-side tables of the chain objective, free of HIP: the SELL-64 arc
// tables of the denominator graph (row order, bank-aware record placement, slice
// ownership), the numerator FSTs' reverse CSR / pdf groups and their packing, the
// graph-size validation, and the LDS sizing formulas and limits the kernels share
// (chain_den.hip includes them from here). Built with the host compiler, so
// tests/test_chain_tables.py runs all of it without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#define DEN_THREADS 1024
#define DEN_WAVES 16
#define DEN_MAXPT 4  // P <= 4096
#define DEN_MAXS 8  // S <= 8192

// fwd / bwd LDS: reduction scratch, the NS-interleaved state row (va or vb, nsl * 64
// entries in the table's slice order) and exp row (xe), and the table's slice metadata
// (len / off / this block's slots)
#define DEN_LDS_TOTAL (160 * 1024)
inline size_t den_rec_fixed_bytes(int P, int nsl, int spg, int ns) {
    return (size_t)4 * (64 + (size_t)ns * ((size_t)nsl * 64 + P + (P & 1)) + 2 * (size_t)nsl + spg) + 64;
}
// posteriors: the alpha' and beta rows of `pair` frames in the f / b tables' slice orders
// (rs = nsl * 64 entries each), the gamma rows and the q table's perm / len / off
inline size_t den_post_lds_bytes(int rs, int P, int nslq, int pair = 1) {
    return (size_t)4 * (64 + 2 * (size_t)pair * rs + (size_t)pair * P + (size_t)nslq * 66);
}

#pragma GCC visibility push(hidden)  // internal to libkaldi_fp16.so

struct SellRec {  // the device's uint2, uploaded byte for byte
    uint32_t x, y;
};
struct Sell {
    std::vector<int> perm, len, off;
    std::vector<SellRec> arcs;
};
// rows of a SELL table keyed by `key`, by non-increasing degree (stable); deg[r] = arcs of row r
std::vector<int> sell_order(int nrows, int A, const int32_t *key, std::vector<int> &deg);
std::vector<int> sell_positions(int nrows, int A, const int32_t *key);
Sell build_sell(int nrows, int A, const int32_t *key, const int32_t *f1, const int32_t *f2,
                const float *tp, int n1, int n2);
void den_balance(const std::vector<int> &len, int G, std::vector<int> &slot, int &spg);
void compute_initial_probs(int S, int A, const int32_t *src, const int32_t *dst, const float *tp,
                   int start, float *out);

// One SELL table with its slice ownership for G = 1 << lg blocks (SellDev::slot / spg;
// empty past the table's last G), and the three tables of a denominator graph
struct DenHostTable {
    Sell sell;
    std::vector<int> slot[4];
    int spg[4];
};
struct DenHost {
    DenHostTable f, b, q;
    int pair_ok;
};
// validates the graph and builds its tables; false with *why set
bool den_host_tables(int S, int P, int A, const int32_t *src, const int32_t *dst, const int32_t *pdf0,
                     const float *tp, DenHost &out, const char **why);
// records with LDS byte offsets for rows interleaving ns sequences or frames
std::vector<SellRec> sell_scaled(const Sell &h, uint32_t ns);

// ---- numerator FST host preparation (reverse CSR + pdf groups) -------------
struct NumHost {  // one FST, local indices
    int S, A, nfinal, start;
    std::vector<int> row_ptr, in_ptr, in_arc, arc_src, arc_dst, arc_pdf, grp_ptr, grp_pdf, grp_arc,
        fin_state, in_src, in_g, arc_g, gsrc, gdst;
    std::vector<float> arc_w, fin_w, in_w, gw;
};

bool prepare_num(NumHost &h, const char **why);
// the numerator tables of a minibatch as one int32 blob; offs[i] = the 19 table offsets of
// FST i inside it
void pack_nums(std::vector<NumHost> &hs, std::vector<int32_t> &blob,
               std::vector<std::vector<size_t>> &offs);

#pragma GCC visibility pop
