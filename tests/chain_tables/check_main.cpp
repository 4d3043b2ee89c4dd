// Stand-alone CPU check of the chain objective's host-side table builders
// (kaldi-fp16_amd/csrc/chain_tables.cpp, linked alone: no HIP). Every check is a property
// stated here from the input arcs, not a digest of the builders' output. Prints one line
// per check, "PASS <subject> <check>" or "FAIL <subject> <check>: <what>", and one
// "REFUSED <case>: <text>" per malformed input; tests/test_chain_tables.py asserts on them.
#include "chain_tables.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <string>

static int g_fail = 0;
static void report(const std::string &subject, const char *check, const std::string &bad) {
    if (bad.empty()) {
        printf("PASS %s %s\n", subject.c_str(), check);
    } else {
        printf("FAIL %s %s: %s\n", subject.c_str(), check, bad.c_str());
        ++g_fail;
    }
}
static std::string at(const char *what, long long i) { return std::string(what) + " at " + std::to_string(i); }

static uint32_t g_rng = 12345;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

struct Graph {
    std::string name;
    int S, P;
    std::vector<int32_t> src, dst, pdf;
    std::vector<float> tp;
    void arc(int s, int d, int p, float w) {
        src.push_back(s);
        dst.push_back(d);
        pdf.push_back(p);
        tp.push_back(w);
    }
    int A() const { return (int)src.size(); }
};

// a ring (every state has an arc in and out) plus `extra` random arcs, all tp > 0
static Graph ring_graph(const char *name, int S, int P, int extra) {
    Graph g{name, S, P, {}, {}, {}, {}};
    for (int s = 0; s < S; ++s) g.arc(s, (s + 1) % S, (int)rnd(P), 0.25f + 0.5f * rnd(100) / 100.0f);
    for (int i = 0; i < extra; ++i) g.arc((int)rnd(S), (int)rnd(S), (int)rnd(P), 0.125f + rnd(100) / 100.0f);
    return g;
}

static std::vector<Graph> graphs() {
    std::vector<Graph> v;
    Graph one{"S1", 1, 1, {}, {}, {}, {}};
    one.arc(0, 0, 0, 1.0f);
    v.push_back(one);
    v.push_back(ring_graph("S31", 31, 5, 70));
    v.push_back(ring_graph("S33", 33, 5, 70));
    v.push_back(ring_graph("S64", 64, 7, 150));
    v.push_back(ring_graph("S65", 65, 7, 150));
    v.push_back(ring_graph("S129", 129, 7, 300));
    Graph skew = ring_graph("skew", 300, 9, 0);  // in-degree 1 everywhere ...
    for (int i = 0; i < 199; ++i) skew.arc((int)rnd(300), 5, (int)rnd(9), 0.5f);  // ... but 200 into state 5
    v.push_back(skew);
    Graph dead{"deadends", 40, 6, {}, {}, {}, {}};  // states 0..4: nothing in; 35..39: nothing out
    for (int i = 0; i < 120; ++i) dead.arc((int)rnd(35), 5 + (int)rnd(35), (int)rnd(6), 0.5f);
    v.push_back(dead);
    v.push_back(ring_graph("P33", 20, 33, 100));
    Graph wide = ring_graph("P4096", 50, 4096, 400);
    wide.pdf[0] = 4095;
    wide.pdf[1] = 0;
    v.push_back(wide);
    return v;
}

typedef std::array<uint32_t, 3> Rec;  // f1, f2, tp bits

// One SELL table against the arcs it was built from: rows = key[a], records {f1[a], f2[a], tp[a]}
static void check_table(const std::string &subject, const Sell &t, int nrows, int A, const int32_t *key,
                        const int32_t *f1, const int32_t *f2, const float *tp, int n1, int n2) {
    const int nsl = (nrows + 63) / 64;
    std::vector<int> deg(nrows, 0);
    for (int a = 0; a < A; ++a) deg[key[a]]++;
    std::string bad;
    // perm: a permutation of the rows by non-increasing degree, stable; -1 behind them
    if ((int)t.perm.size() != nsl * 64) bad = "perm size";
    std::vector<int> seen(nrows, 0);
    for (int r = 0; r < nsl * 64 && bad.empty(); ++r) {
        const int p = t.perm[r];
        if (r >= nrows) {
            if (p != -1) bad = at("tail not -1", r);
            continue;
        }
        if (p < 0 || p >= nrows || seen[p]++) bad = at("not a permutation", r);
        else if (r && deg[t.perm[r - 1]] < deg[p]) bad = at("degree increases", r);
        else if (r && deg[t.perm[r - 1]] == deg[p] && t.perm[r - 1] > p) bad = at("not stable", r);
    }
    report(subject, "perm", bad);
    if (!bad.empty()) return;
    // len / off
    bad.clear();
    if ((int)t.len.size() != nsl || (int)t.off.size() != nsl) bad = "len/off size";
    int tot = 0;
    for (int j = 0; j < nsl && bad.empty(); ++j) {
        int mx = 0;
        for (int r = j * 64; r < std::min(nrows, j * 64 + 64); ++r) mx = std::max(mx, deg[t.perm[r]]);
        if (t.len[j] % 8 || t.len[j] < mx) bad = at("len", j);
        if (t.off[j] != tot) bad = at("off", j);
        tot += t.len[j];
    }
    if (bad.empty() && t.arcs.size() != (size_t)tot * 64) bad = "arcs size";
    report(subject, "len_off", bad);
    if (!bad.empty()) return;
    // records: per row the multiset of its arcs; everything else is padding with tp = 0
    // on valid indices (the graphs have tp > 0 on every arc)
    std::string badrec, badpad;
    std::vector<std::vector<Rec>> want(nrows);
    for (int a = 0; a < A; ++a) {
        uint32_t bits;
        memcpy(&bits, &tp[a], 4);
        want[key[a]].push_back(Rec{(uint32_t)f1[a], (uint32_t)f2[a], bits});
    }
    for (int r = 0; r < nsl * 64; ++r) {
        const int j = r / 64, l = r % 64;
        std::vector<Rec> got;
        for (int k = 0; k < t.len[j]; ++k) {
            const SellRec &x = t.arcs[((size_t)t.off[j] + k) * 64 + l];
            const uint32_t a1 = x.x & 0xFFFF, a2 = x.x >> 16;
            if (x.y != 0) got.push_back(Rec{a1, a2, x.y});
            else if ((int)a1 >= n1 || (int)a2 >= n2) badpad = at("padding index out of range, row", r);
        }
        std::vector<Rec> w = r < nrows ? want[t.perm[r]] : std::vector<Rec>();
        std::sort(got.begin(), got.end());
        std::sort(w.begin(), w.end());
        if (got != w && badrec.empty()) badrec = at("records differ from the row's arcs, row", r);
    }
    report(subject, "records", badrec);
    report(subject, "padding", badpad);
    // sell_positions is the inverse of perm
    bad.clear();
    const std::vector<int> pos = sell_positions(nrows, A, key);
    for (int r = 0; r < nrows && bad.empty(); ++r)
        if (pos[t.perm[r]] != r) bad = at("position", r);
    report(subject, "positions", bad);
    // scaled records: 4 * ns * f in both halves, each inside its 16 bits
    bad.clear();
    for (uint32_t ns = 1; ns <= 2 && bad.empty(); ++ns) {
        const std::vector<SellRec> sc = sell_scaled(t, ns);
        if (sc.size() != t.arcs.size()) bad = "size";
        for (size_t i = 0; i < sc.size() && bad.empty(); ++i) {
            const uint32_t a1 = t.arcs[i].x & 0xFFFF, a2 = t.arcs[i].x >> 16;
            if (4 * ns * a1 >= 65536 || 4 * ns * a2 >= 65536) bad = at("offset past 16 bits", (long long)i);
            else if ((sc[i].x & 0xFFFF) != 4 * ns * a1 || (sc[i].x >> 16) != 4 * ns * a2 || sc[i].y != t.arcs[i].y)
                bad = at("scaled record", (long long)i);
        }
    }
    report(subject, "scaled", bad);
}

// slice ownership: slot[gi * spg + k] is slot k of block gi, run by wave k % DEN_WAVES
static std::string check_balance(const std::vector<int> &len, int G, const std::vector<int> &slot, int spg) {
    const int nsl = (int)len.size();
    if (spg <= 0 || spg % DEN_WAVES) return "spg not a multiple of DEN_WAVES";
    if (slot.size() != (size_t)G * spg) return "slot size";
    std::vector<int> owners(nsl, 0);
    std::vector<long long> load((size_t)G * DEN_WAVES, 0);
    long long total = 0, biggest = 0;
    for (int gi = 0; gi < G; ++gi)
        for (int k = 0; k < spg; ++k) {
            const int j = slot[(size_t)gi * spg + k];
            if (j == -1) continue;
            if (j < 0 || j >= nsl) return at("slot value", (long long)gi * spg + k);
            owners[j]++;
            load[(size_t)gi * DEN_WAVES + k % DEN_WAVES] += len[j] + 4;
        }
    for (int j = 0; j < nsl; ++j) {
        if (owners[j] != 1) return at("slice not owned exactly once", j);
        total += len[j] + 4;
        biggest = std::max<long long>(biggest, len[j] + 4);
    }
    // greedy bound: the fullest bin was the emptiest (at most the mean) before its last slice
    const long long mx = *std::max_element(load.begin(), load.end());
    if (mx * (long long)load.size() > total + biggest * (long long)load.size()) return "load above mean + largest";
    return "";
}

static void check_graph(const Graph &g) {
    DenHost h;
    const char *why = nullptr;
    const int A = g.A();
    if (!den_host_tables(g.S, g.P, A, g.src.data(), g.dst.data(), g.pdf.data(), g.tp.data(), h, &why)) {
        report(g.name, "accepted", why ? why : "(no text)");
        return;
    }
    report(g.name, "accepted", "");
    const int rs = (g.S + 63) / 64 * 64;
    const std::vector<int> posf = sell_positions(g.S, A, g.dst.data()), posb = sell_positions(g.S, A, g.src.data());
    std::vector<int32_t> src_f(A), dst_b(A);
    for (int a = 0; a < A; ++a) {
        src_f[a] = posf[g.src[a]];
        dst_b[a] = posb[g.dst[a]];
    }
    check_table(g.name + ".f", h.f.sell, g.S, A, g.dst.data(), src_f.data(), g.pdf.data(), g.tp.data(), rs, g.P);
    check_table(g.name + ".b", h.b.sell, g.S, A, g.src.data(), dst_b.data(), g.pdf.data(), g.tp.data(), rs, g.P);
    check_table(g.name + ".q", h.q.sell, g.P, A, g.pdf.data(), src_f.data(), dst_b.data(), g.tp.data(), rs, rs);
    std::string bad;
    const DenHostTable *tabs[3] = {&h.f, &h.b, &h.q};
    for (int i = 0; i < 3 && bad.empty(); ++i)
        for (int lg = 0; lg < (i == 2 ? 1 : 4) && bad.empty(); ++lg)
            bad = check_balance(tabs[i]->sell.len, 1 << lg, tabs[i]->slot[lg], tabs[i]->spg[lg]);
    report(g.name, "ownership", bad);
}

static void check_den_balance() {
    for (int nsl : {1, 15, 16, 17, 111})
        for (int G : {1, 2, 4, 8}) {
            std::vector<int> len(nsl);
            for (int j = 0; j < nsl; ++j) len[j] = 8 * (1 + (j * j * 7) % 23);
            len[nsl / 2] = 8 * 200;  // one slice far above the rest
            std::vector<int> slot;
            int spg = 0;
            den_balance(len, G, slot, spg);
            report("balance.nsl" + std::to_string(nsl) + ".G" + std::to_string(G), "slots", check_balance(len, G, slot, spg));
        }
}

// ---- numerator FSTs ---------------------------------------------------------
static NumHost fst(int S, std::vector<int> row_ptr, std::vector<int> dst, std::vector<int> pdf, std::vector<int> fin) {
    NumHost h;
    h.S = S;
    h.A = (int)dst.size();
    h.start = 0;
    h.row_ptr = row_ptr;
    h.arc_dst = dst;
    h.arc_pdf = pdf;
    for (int a = 0; a < h.A; ++a) h.arc_w.push_back(-0.25f * (a + 1));
    h.fin_state = fin;
    h.nfinal = (int)fin.size();
    for (int i = 0; i < h.nfinal; ++i) h.fin_w.push_back(-0.5f * (i + 1));
    return h;
}

static std::vector<std::pair<std::string, NumHost>> fsts() {
    return {
        {"one_state", fst(1, {0, 1}, {0}, {3}, {0})},
        {"chain", fst(5, {0, 1, 2, 3, 4, 4}, {1, 2, 3, 4}, {2, 9, 2, 1}, {4})},
        // a lattice with epsilon arcs (pdf 0 and -1), repeated pdfs and parallel arcs
        {"lattice", fst(6, {0, 3, 5, 8, 10, 11, 11}, {1, 2, 1, 3, 2, 3, 4, 3, 4, 5, 5},
                        {4, 0, 2, 4, -1, 2, 7, 0, 4, 2, 7}, {5, 4})},
    };
}

static std::string check_prepared(const NumHost &h) {
    const int S = h.S, A = h.A;
    if ((int)h.arc_src.size() != A || (int)h.in_ptr.size() != S + 1 || (int)h.in_arc.size() != A) return "sizes";
    for (int s = 0; s < S; ++s)
        for (int a = h.row_ptr[s]; a < h.row_ptr[s + 1]; ++a)
            if (h.arc_src[a] != s) return at("arc_src", a);
    // in_arc: the incoming arcs of every state, in arc-index order
    if (h.in_ptr[0] != 0 || h.in_ptr[S] != A) return "in_ptr ends";
    for (int d = 0; d < S; ++d) {
        std::vector<int> want;
        for (int a = 0; a < A; ++a)
            if (h.arc_dst[a] == d) want.push_back(a);
        if (h.in_ptr[d + 1] - h.in_ptr[d] != (int)want.size()) return at("in_ptr", d);
        if (!std::equal(want.begin(), want.end(), h.in_arc.begin() + h.in_ptr[d])) return at("in_arc order", d);
    }
    // groups: pdfs > 0 ascending, each group's arcs in arc-index order
    const int G = (int)h.grp_pdf.size();
    if ((int)h.grp_ptr.size() != G + 1 || h.grp_ptr[0] != 0 || h.grp_ptr[G] != (int)h.grp_arc.size()) return "grp_ptr";
    int npos = 0;
    for (int a = 0; a < A; ++a) npos += h.arc_pdf[a] > 0;
    if ((int)h.grp_arc.size() != npos) return "grp_arc does not hold every arc with a pdf once";
    if ((int)h.arc_g.size() != A) return "arc_g size";
    std::vector<int> grp_of(A, -1);
    for (int q = 0; q < G; ++q) {
        if (h.grp_pdf[q] <= 0 || (q && h.grp_pdf[q - 1] >= h.grp_pdf[q])) return at("grp_pdf order", q);
        if (h.grp_ptr[q + 1] <= h.grp_ptr[q]) return at("empty group", q);
        for (int k = h.grp_ptr[q]; k < h.grp_ptr[q + 1]; ++k) {
            const int a = h.grp_arc[k];
            if (a < 0 || a >= A || h.arc_pdf[a] != h.grp_pdf[q] || grp_of[a] != -1) return at("grp_arc", k);
            if (k > h.grp_ptr[q] && h.grp_arc[k - 1] >= a) return at("grp_arc order", k);
            grp_of[a] = q;
        }
    }
    for (int a = 0; a < A; ++a)
        if (h.arc_g[a] != grp_of[a]) return at("arc_g", a);
    // the gathers
    if ((int)h.in_src.size() != A || (int)h.in_g.size() != A || (int)h.in_w.size() != A) return "in_* sizes";
    for (int k = 0; k < A; ++k) {
        const int a = h.in_arc[k];
        if (h.in_src[k] != h.arc_src[a] || h.in_g[k] != h.arc_g[a] || h.in_w[k] != h.arc_w[a]) return at("in_* gather", k);
    }
    if ((int)h.gsrc.size() != npos || (int)h.gdst.size() != npos || (int)h.gw.size() != npos) return "g* sizes";
    for (int k = 0; k < npos; ++k) {
        const int a = h.grp_arc[k];
        if (h.gsrc[k] != h.arc_src[a] || h.gdst[k] != h.arc_dst[a] || h.gw[k] != h.arc_w[a]) return at("g* gather", k);
    }
    return "";
}

template <typename T>
static bool blob_holds(const std::vector<int32_t> &blob, size_t off, const std::vector<T> &v) {
    return off + v.size() <= blob.size() && (v.empty() || !memcmp(blob.data() + off, v.data(), v.size() * 4));
}

static void check_nums() {
    std::vector<NumHost> hs;
    for (auto &nf : fsts()) {
        const char *why = nullptr;
        NumHost h = nf.second;
        if (!prepare_num(h, &why)) {
            report("num." + nf.first, "prepared", why ? why : "(no text)");
            continue;
        }
        report("num." + nf.first, "prepared", check_prepared(h));
        hs.push_back(h);
    }
    // the 19 tables of every FST tile the blob in the documented order, without gaps
    std::vector<int32_t> blob;
    std::vector<std::vector<size_t>> offs;
    pack_nums(hs, blob, offs);
    std::string bad;
    size_t next = 0;
    if (offs.size() != hs.size()) bad = "offs size";
    for (size_t i = 0; i < hs.size() && bad.empty(); ++i) {
        const NumHost &h = hs[i];
        const std::vector<int> *iv[] = {&h.row_ptr, &h.in_ptr, &h.in_arc, &h.arc_src, &h.arc_dst, &h.arc_pdf, nullptr,
                                        &h.grp_ptr, &h.grp_pdf, &h.grp_arc, &h.fin_state, nullptr, &h.in_src,
                                        &h.in_g, &h.arc_g, &h.gsrc, &h.gdst, nullptr, nullptr};
        const std::vector<float> *fv[] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &h.arc_w,
                                          nullptr, nullptr, nullptr, nullptr, &h.fin_w, nullptr,
                                          nullptr, nullptr, nullptr, nullptr, &h.in_w, &h.gw};
        if (offs[i].size() != 19) {
            bad = at("not 19 offsets, FST", (long long)i);
            break;
        }
        for (int k = 0; k < 19 && bad.empty(); ++k) {
            if (offs[i][k] != next) bad = at("gap or overlap before table", (long long)i * 19 + k);
            else if (iv[k] ? !blob_holds(blob, next, *iv[k]) : !blob_holds(blob, next, *fv[k]))
                bad = at("table contents", (long long)i * 19 + k);
            next += iv[k] ? iv[k]->size() : fv[k]->size();
        }
    }
    if (bad.empty() && next != blob.size()) bad = "blob longer than its tables";
    report("num.pack", "tiles", bad);
    // malformed inputs
    struct Bad {
        const char *name;
        NumHost h;
    } bads[] = {
        {"row_ptr_not_monotone", fst(3, {0, 2, 1, 2}, {1, 2}, {1, 2}, {2})},
        {"destination_out_of_range", fst(2, {0, 1, 1}, {2}, {1}, {1})},
        {"final_out_of_range", fst(2, {0, 1, 1}, {1}, {1}, {2})},
        {"row_ptr_end", fst(2, {0, 1, 1}, {1, 1}, {1, 1}, {1})},
    };
    for (auto &b : bads) {
        const char *why = nullptr;
        if (prepare_num(b.h, &why)) printf("FAIL num.%s refused: accepted\n", b.name), ++g_fail;
        else printf("REFUSED num.%s: %s\n", b.name, why ? why : "(no text)");
    }
}

static void check_initial_probs() {
    {  // 0 -> 0 (1/2), 0 -> 1 (1/2), 1 -> 0 (1): p_t(1) = (1 - (-1/2)^t) / 3, averaged over t = 0..99
        const int32_t src[] = {0, 0, 1}, dst[] = {0, 1, 0};
        const float tp[] = {0.5f, 0.5f, 1.0f};
        float out[2];
        compute_initial_probs(2, 3, src, dst, tp, 0, out);
        const double want1 = (1.0 - (1.0 - pow(-0.5, 100)) / 1.5 / 100.0) / 3.0;
        std::string bad;
        if (fabs((double)out[0] + out[1] - 1.0) > 1e-6) bad = "sum " + std::to_string(out[0] + out[1]);
        else if (fabs(out[1] - want1) > 1e-6) bad = "state 1: " + std::to_string(out[1]);
        report("initial_probs.two_state", "closed_form", bad);
    }
    {  // 0 -> 1 -> 2 and nothing leaves 2: the mass is gone after three steps (tot == 0)
        const int32_t src[] = {0, 1}, dst[] = {1, 2};
        const float tp[] = {1.0f, 1.0f};
        float out[3];
        compute_initial_probs(3, 2, src, dst, tp, 0, out);
        std::string bad;
        for (int s = 0; s < 3; ++s)
            if (!(out[s] >= 0.0f && out[s] <= 1.0f)) bad = at("not a finite probability", s);
        report("initial_probs.dead_end", "finite", bad);
    }
}

static void check_limits() {
    struct Case {
        const char *name;
        int S, P;
        float tp;
    } cases[] = {{"S65536", 65536, 4, 0.5f}, {"P4097", 4, 4097, 0.5f}, {"negative_tp", 4, 4, -0.5f}, {"nan_tp", 4, 4, NAN}};
    for (auto &c : cases) {
        const int32_t src[] = {0, 1}, dst[] = {1, 0}, pdf[] = {0, 1};
        const float tp[] = {0.5f, c.tp};
        DenHost h;
        const char *why = nullptr;
        if (den_host_tables(c.S, c.P, 2, src, dst, pdf, tp, h, &why)) printf("FAIL den.%s refused: accepted\n", c.name), ++g_fail;
        else printf("REFUSED den.%s: %s\n", c.name, why ? why : "(no text)");
    }
}

int main() {
    for (const Graph &g : graphs()) check_graph(g);
    check_den_balance();
    check_nums();
    check_initial_probs();
    check_limits();
    printf("DONE %d failure(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
