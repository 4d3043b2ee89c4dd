// chain_tables.cpp — the chain objective's host-side table builders (chain_tables.h): pure
// CPU algorithms, no HIP. Every numerical property of the denominator follows from them:
// the per-row summation order, the placement of records within a slice step, the tp = 0
// padding records on valid indices, and each slice's single owner.
#include "chain_tables.h"

#include <string.h>

#include <algorithm>

// ===========================================================================
// SELL-64 tables of the denominator graph
// ===========================================================================
std::vector<int> sell_order(int nrows, int A, const int32_t *key, std::vector<int> &deg) {
    deg.assign(nrows, 0);
    std::vector<int> order(nrows);
    for (int a = 0; a < A; ++a) deg[key[a]]++;
    for (int i = 0; i < nrows; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return deg[a] > deg[b]; });
    return order;
}

// slice position of every row of a SELL table keyed by `key` (rows sorted by degree,
// stable: the order build_sell uses)
std::vector<int> sell_positions(int nrows, int A, const int32_t *key) {
    std::vector<int> deg, pos(nrows);
    const std::vector<int> order = sell_order(nrows, A, key, deg);
    for (int i = 0; i < nrows; ++i) pos[order[i]] = i;
    return pos;
}

// rows = values of key[] in [0, nrows); each row lists {f1 | f2<<16, tp} in arc order
Sell build_sell(int nrows, int A, const int32_t *key, const int32_t *f1, const int32_t *f2,
                const float *tp, int n1, int n2) {
    Sell s;
    std::vector<int> deg;
    const std::vector<int> order = sell_order(nrows, A, key, deg);
    const int nsl = (nrows + 63) / 64;
    s.perm.assign((size_t)nsl * 64, -1);
    s.len.resize(nsl);
    s.off.resize(nsl);
    std::vector<int> rowpos(nrows);
    int tot = 0;
    for (int j = 0; j < nsl; ++j) {
        int mx = 0;
        for (int l = 0; l < 64; ++l) {
            int r = j * 64 + l;
            if (r < nrows) {
                s.perm[r] = order[r];
                rowpos[order[r]] = r;
                mx = std::max(mx, deg[order[r]]);
            }
        }
        mx = (mx + 7) & ~7;  // whole 8-record steps; the padding records have tp = 0
        s.len[j] = mx;
        s.off[j] = tot;
        tot += mx;
    }
    s.arcs.assign((size_t)tot * 64, SellRec{0u, 0u});  // tp = 0 padding
    // arcs of every row, in arc order
    std::vector<std::vector<int>> rows(nrows);
    for (int a = 0; a < A; ++a) rows[key[a]].push_back(a);
    // Place each row's arcs into the slice's steps so that, per step and per
    // 32-lane half-wave, the two LDS gathers (f1 and f2 indices) fall in distinct
    // banks ((index) mod 32 for ds_read_b32) as far as possible; padding records
    // (tp = 0) take indices of free banks. Summation order per row changes, but
    // stays fixed.
    for (int j = 0; j < nsl; ++j) {
        for (int half = 0; half < 2; ++half) {
            std::vector<std::vector<int>> rem(32);
            for (int l = 0; l < 32; ++l) {
                int r = j * 64 + half * 32 + l;
                if (r < nrows) rem[l] = rows[s.perm[r]];
            }
            for (int k = 0; k < s.len[j]; ++k) {
                bool used1[32] = {false}, used2[32] = {false};
                // rows with the most remaining arcs choose first
                int order[32];
                for (int l = 0; l < 32; ++l) order[l] = l;
                std::stable_sort(order, order + 32,
                                 [&](int x, int y) { return rem[x].size() > rem[y].size(); });
                for (int oi = 0; oi < 32; ++oi) {
                    const int l = order[oi];
                    SellRec rec{0u, 0u};
                    if (!rem[l].empty()) {
                        size_t best = 0;
                        int bestc = 3;
                        for (size_t q = 0; q < rem[l].size() && bestc > 0; ++q) {
                                const int a = rem[l][q];
                                int c = (used1[f1[a] & 31] ? 1 : 0) + (used2[f2[a] & 31] ? 1 : 0);
                                if (c < bestc) {
                                    bestc = c;
                                    best = q;
                                }
                            }
                        const int a = rem[l][best];
                        rem[l].erase(rem[l].begin() + best);
                        used1[f1[a] & 31] = used2[f2[a] & 31] = true;
                        uint32_t tpu;
                        memcpy(&tpu, &tp[a], 4);
                        rec = SellRec{(uint32_t)f1[a] | ((uint32_t)f2[a] << 16), tpu};
                    } else {  // padding: valid indices on free banks
                        const int m1 = std::min(32, n1) - 1, m2 = std::min(32, n2) - 1;
                        int b1 = 0, b2 = 0;
                        while (b1 < m1 && used1[b1]) ++b1;
                        while (b2 < m2 && used2[b2]) ++b2;
                        used1[b1] = used2[b2] = true;
                        rec = SellRec{(uint32_t)b1 | ((uint32_t)b2 << 16), 0u};
                    }
                    s.arcs[((size_t)s.off[j] + k) * 64 + half * 32 + l] = rec;
                }
            }
        }
    }
    return s;
}

// Slice ownership of SellDev::slot for G blocks of DEN_WAVES waves: longest
// slice first onto the least loaded (block, wave) pair (a slice costs its rows plus a
// fixed 4 for its per-slice work); bin b is block b % G, wave b / G, so the largest
// slices also spread over the blocks.
void den_balance(const std::vector<int> &len, int G, std::vector<int> &slot, int &spg) {
    const int nsl = (int)len.size(), bins = G * DEN_WAVES;
    std::vector<int> order(nsl);
    for (int j = 0; j < nsl; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
    std::vector<long long> load(bins, 0);
    std::vector<std::vector<int>> lists(bins);
    for (int j : order) {
        int b = 0;
        for (int i = 1; i < bins; ++i)
            if (load[i] < load[b]) b = i;
        lists[b].push_back(j);
        load[b] += len[j] + 4;
    }
    size_t maxc = 1;
    for (auto &l : lists) maxc = std::max(maxc, l.size());
    spg = (int)maxc * DEN_WAVES;
    slot.assign((size_t)G * spg, -1);
    for (int b = 0; b < bins; ++b) {
        const int gi = b % G, w = b / G;
        for (size_t i = 0; i < lists[b].size(); ++i) slot[(size_t)gi * spg + w + DEN_WAVES * (int)i] = lists[b][i];
    }
}

bool den_host_tables(int S, int P, int A, const int32_t *src, const int32_t *dst, const int32_t *pdf0,
                     const float *tp, DenHost &out, const char **why) {
    if (S <= 0 || P <= 0 || A <= 0) {
        *why = "empty denominator graph";
        return false;
    }
    if (S > 65535 || P > 65535) {
        *why = "den graph needs num_states, num_pdfs <= 65535 (16-bit arc fields)";
        return false;
    }
    if (P > DEN_MAXPT * DEN_THREADS) {
        *why = "num_pdfs > 4096 not supported";
        return false;
    }
    // S < 8192: the pair records hold 8 * (slice position) as a 16-bit LDS byte offset
    const int rsS = (S + 63) / 64 * 64;
    if (den_post_lds_bytes(rsS, P, (P + 63) / 64) > DEN_LDS_TOTAL ||
        den_rec_fixed_bytes(P, (S + 63) / 64, (S + 63) / 64, 1) > DEN_LDS_TOTAL || S >= DEN_MAXS * DEN_THREADS) {
        *why = "den graph too large for the LDS-resident kernels (S < 8192, ~12*S + 14*P B)";
        return false;
    }
    for (int a = 0; a < A; ++a)
        if (src[a] < 0 || src[a] >= S || dst[a] < 0 || dst[a] >= S || pdf0[a] < 0 ||
            pdf0[a] >= P || !(tp[a] >= 0.0f)) {
            *why = "den transition out of range (state, pdf or negative probability)";
            return false;
        }
    // The recursions and the posteriors keep their state rows in LDS in the f (alpha') and
    // b (beta) tables' slice orders, the layout the stores use: the records name states
    // by slice position, so the per-frame row copies into LDS are linear (no permutation,
    // no bank conflicts) and the padding positions hold zeros (or, in beta rows, values
    // only tp = 0 padding records read).
    const std::vector<int> posf = sell_positions(S, A, dst), posb = sell_positions(S, A, src);
    std::vector<int32_t> src_f(A), dst_b(A);
    for (int a = 0; a < A; ++a) {
        src_f[a] = posf[src[a]];
        dst_b[a] = posb[dst[a]];
    }
    out.f.sell = build_sell(S, A, dst, src_f.data(), pdf0, tp, rsS, P);
    out.b.sell = build_sell(S, A, src, dst_b.data(), pdf0, tp, rsS, P);
    out.q.sell = build_sell(P, A, pdf0, src_f.data(), dst_b.data(), tp, rsS, rsS);
    auto own = [](DenHostTable &t, int ngs) {
        for (int lg = 0; lg < 4; ++lg) {
            t.slot[lg].clear();
            t.spg[lg] = 0;
            if (lg < ngs) den_balance(t.sell.len, 1 << lg, t.slot[lg], t.spg[lg]);
        }
    };
    own(out.f, 4);
    own(out.b, 4);
    own(out.q, 1);
    out.pair_ok = 1;
    const int nslf = (int)out.f.sell.len.size();
    for (int lg = 0; lg < 4; ++lg) {
        const int spg = std::max(out.f.spg[lg], out.b.spg[lg]);
        if (den_rec_fixed_bytes(P, nslf, spg, 1) > DEN_LDS_TOTAL) {
            *why = "den graph too large for the LDS-resident kernels (slice lists)";
            return false;
        }
        if (den_rec_fixed_bytes(P, nslf, spg, 2) > DEN_LDS_TOTAL) out.pair_ok = 0;
    }
    return true;
}

// records with LDS byte offsets for the interleaved rows (den_fwd_body / den_bwd_body,
// k_den_post)
std::vector<SellRec> sell_scaled(const Sell &h, uint32_t ns) {
    std::vector<SellRec> a(h.arcs);
    for (auto &r : a) {
        const uint32_t f1 = r.x & 0xFFFF, f2 = r.x >> 16;
        r.x = (4 * ns * f1) | ((4 * ns * f2) << 16);
    }
    return a;
}

// denominator.go:131-171
void compute_initial_probs(int S, int A, const int32_t *src, const int32_t *dst, const float *tp,
                   int start, float *out) {
    std::vector<double> cur(S, 0.0), next(S, 0.0), avg(S, 0.0);
    cur[start] = 1.0;
    for (int it = 0; it < 100; ++it) {
        for (int s = 0; s < S; ++s) avg[s] += cur[s] / 100.0;
        std::fill(next.begin(), next.end(), 0.0);
        for (int a = 0; a < A; ++a) next[dst[a]] += cur[src[a]] * (double)tp[a];
        double tot = 0.0;
        for (int s = 0; s < S; ++s) tot += next[s];
        if (tot > 0) {
            double inv = 1.0 / tot;
            for (int s = 0; s < S; ++s) next[s] *= inv;
        }
        cur.swap(next);
    }
    for (int s = 0; s < S; ++s) out[s] = (float)avg[s];
}

// ===========================================================================
// Numerator FSTs: reverse CSR, pdf groups, packing
// ===========================================================================
bool prepare_num(NumHost &h, const char **why) {
    const int S = h.S, A = h.A;
    if (S <= 0) {
        *why = "FST has no states";
        return false;
    }
    if ((int)h.row_ptr.size() != S + 1 || h.row_ptr[0] != 0 || h.row_ptr[S] != A) {
        *why = "row_ptr does not describe num_arcs arcs";
        return false;
    }
    h.arc_src.assign(A, 0);
    for (int s = 0; s < S; ++s) {
        if (h.row_ptr[s + 1] < h.row_ptr[s]) {
            *why = "row_ptr not monotone";
            return false;
        }
        for (int a = h.row_ptr[s]; a < h.row_ptr[s + 1]; ++a) h.arc_src[a] = s;
    }
    for (int a = 0; a < A; ++a)
        if (h.arc_dst[a] < 0 || h.arc_dst[a] >= S) {
            *why = "arc destination out of range";
            return false;
        }
    for (int i = 0; i < h.nfinal; ++i)
        if (h.fin_state[i] < 0 || h.fin_state[i] >= S) {
            *why = "final state out of range";
            return false;
        }
    if (h.start < 0 || h.start >= S) {
        *why = "start state out of range";
        return false;
    }
    // reverse CSR, incoming arcs in arc-index order (chain_det.cu:243-290)
    h.in_ptr.assign(S + 1, 0);
    for (int a = 0; a < A; ++a) h.in_ptr[h.arc_dst[a] + 1]++;
    for (int s = 0; s < S; ++s) h.in_ptr[s + 1] += h.in_ptr[s];
    h.in_arc.assign(A, 0);
    std::vector<int> pos(h.in_ptr.begin(), h.in_ptr.end() - 1);
    for (int a = 0; a < A; ++a) h.in_arc[pos[h.arc_dst[a]]++] = a;
    // pdf groups, arcs in arc-index order inside each group
    std::vector<int> idx;
    for (int a = 0; a < A; ++a)
        if (h.arc_pdf[a] > 0) idx.push_back(a);
    std::stable_sort(idx.begin(), idx.end(),
                     [&](int x, int y) { return h.arc_pdf[x] < h.arc_pdf[y]; });
    h.grp_ptr.assign(1, 0);
    h.grp_pdf.clear();
    h.grp_arc = idx;
    for (size_t i = 0; i < idx.size(); ++i) {
        if (i == 0 || h.arc_pdf[idx[i]] != h.arc_pdf[idx[i - 1]]) {
            if (i) h.grp_ptr.push_back((int)i);
            h.grp_pdf.push_back(h.arc_pdf[idx[i]]);
        }
    }
    if (!idx.empty()) h.grp_ptr.push_back((int)idx.size());
    // pre-gathered arc fields for k_num_fb
    h.arc_g.assign(A, -1);
    for (size_t q = 0; q + 1 < h.grp_ptr.size(); ++q)
        for (int k = h.grp_ptr[q]; k < h.grp_ptr[q + 1]; ++k) h.arc_g[h.grp_arc[k]] = (int)q;
    h.in_src.resize(A);
    h.in_g.resize(A);
    h.in_w.resize(A);
    for (int k = 0; k < A; ++k) {
        int a = h.in_arc[k];
        h.in_src[k] = h.arc_src[a];
        h.in_g[k] = h.arc_g[a];
        h.in_w[k] = h.arc_w[a];
    }
    h.gsrc.resize(idx.size());
    h.gdst.resize(idx.size());
    h.gw.resize(idx.size());
    for (size_t k = 0; k < idx.size(); ++k) {
        h.gsrc[k] = h.arc_src[idx[k]];
        h.gdst[k] = h.arc_dst[idx[k]];
        h.gw[k] = h.arc_w[idx[k]];
    }
    return true;
}

template <typename T>
static void append(std::vector<int32_t> &blob, const std::vector<T> &v, std::vector<size_t> &offs) {
    offs.push_back(blob.size());
    size_t n = blob.size();
    blob.resize(n + v.size());
    if (!v.empty()) memcpy(blob.data() + n, v.data(), v.size() * 4);
}

// the numerator tables of a minibatch as one int32 blob; offs[i] = the 19 table offsets of
// FST i inside it
void pack_nums(std::vector<NumHost> &hs, std::vector<int32_t> &blob,
               std::vector<std::vector<size_t>> &offs) {
    blob.clear();
    offs.assign(hs.size(), {});
    for (size_t i = 0; i < hs.size(); ++i) {
        NumHost &h = hs[i];
        auto &o = offs[i];
        append(blob, h.row_ptr, o);
        append(blob, h.in_ptr, o);
        append(blob, h.in_arc, o);
        append(blob, h.arc_src, o);
        append(blob, h.arc_dst, o);
        append(blob, h.arc_pdf, o);
        append(blob, h.arc_w, o);
        append(blob, h.grp_ptr, o);
        append(blob, h.grp_pdf, o);
        append(blob, h.grp_arc, o);
        append(blob, h.fin_state, o);
        append(blob, h.fin_w, o);
        append(blob, h.in_src, o);
        append(blob, h.in_g, o);
        append(blob, h.arc_g, o);
        append(blob, h.gsrc, o);
        append(blob, h.gdst, o);
        append(blob, h.in_w, o);
        append(blob, h.gw, o);
    }
}
