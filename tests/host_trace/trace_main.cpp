// trace_main.cpp — drives the host layer (nnet_*) over the stub backend and prints, per
// scenario, the C-ABI calls it made (stub_backend.cpp) and the error texts of the negative
// cases. usage: host_trace <configs dir>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <dirent.h>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/bridge.h"
#include "../../include/kf_nnet.h"

extern "C" void stub_reset(void);

namespace {

std::string g_dir;

// tiny.xconfig itself cannot take the row-subsampled step (tdnnf8 has time stride 1, so
// nnet_set_row_subsampling refuses it); "tiny_s3" is tiny with that stride set to 3
const char *const kTinyS3 = "tiny_s3";
// further variants of tiny, by text replacement: a dropout component on every tdnnf-layer (the
// replacement of tests/test_gpu_dropout_net.py), that on tiny_s3, and a spec-augment-layer
// between tdnnf5 and tdnnf6 (its consumer reads an MXFP8 copy in MXFP8 mode)
const char *const kTinyDrop = "tiny_drop", *const kTinyS3Drop = "tiny_s3_drop", *const kTinySaMid = "tiny_sa_mid";
const char *const kTinySa = "specaug/tiny_specaug.xconfig";

std::string replaced(std::string t, const std::string &from, const std::string &to) {
    size_t at = t.find(from), n = 0;
    for (; at != std::string::npos; at = t.find(from, at + to.size()), ++n) t.replace(at, from.size(), to);
    if (!n) exit(2);
    return t;
}

std::string read_cfg(const std::string &name) {
    if (name == kTinyS3) return replaced(read_cfg("tiny.xconfig"), "time-stride=1", "time-stride=3");
    if (name == kTinyDrop || name == kTinyS3Drop)
        return replaced(read_cfg(name == kTinyDrop ? "tiny.xconfig" : kTinyS3), "bypass-scale=0.66",
                        "bypass-scale=0.66 dropout-proportion=0.0");
    if (name == kTinySaMid)
        return replaced(read_cfg("tiny.xconfig"), "tdnnf-layer name=tdnnf6",
                        "spec-augment-layer name=mid-spec-augment\ntdnnf-layer name=tdnnf6");
    std::ifstream f(g_dir + "/" + name);
    if (!f) {
        fprintf(stderr, "cannot read %s/%s\n", g_dir.c_str(), name.c_str());
        exit(2);
    }
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

void scenario(const std::string &name) {
    stub_reset();
    printf("== scenario %s\n", name.c_str());
}
// an nnet_* call's status, with the error text when it failed
void rc(const char *what, int r) {
    if (r == 0) {
        printf("-- %s ok\n", what);
    } else {
        const char *e = nnet_last_error();
        printf("-- %s rc=%d error: %s\n", what, r, e ? e : "(none)");
    }
}

struct Run {
    KfNet *net = nullptr;
    void *feats = nullptr, *ograd = nullptr, *ivec = nullptr;
    bool is_ivec = false;
    int T = 0;

    Run(const std::string &cfg, int max_frames) {
        const std::string text = read_cfg(cfg);
        net = nnet_create(text.c_str(), max_frames);
        if (!net) {
            printf("-- create failed: %s\n", nnet_last_error() ? nnet_last_error() : "(none)");
            return;
        }
        is_ivec = text.find("name=ivector ") != std::string::npos;
        feats = bridge_gpu_malloc((size_t)max_frames * 4096);
        ograd = bridge_gpu_malloc((size_t)max_frames * 16384);
        ivec = bridge_gpu_malloc(4096);
        std::vector<float> p((size_t)nnet_num_params(net));
        for (size_t i = 0; i < p.size(); ++i) p[i] = 0.01f * (float)((int)(i % 7) - 3);
        rc("set_params", nnet_set_params(net, p.data()));
    }
    ~Run() {
        if (net) nnet_free(net);
    }
    void forward(int frames) {
        T = frames;
        if (is_ivec) {
            const int seq[3] = {0, frames / 2, frames};
            rc("forward_ivector", nnet_forward_ivector(net, feats, frames, ivec, 2, seq));
        } else {
            rc("forward", nnet_forward(net, feats, frames));
        }
        int tc = 0, tc0 = 0;
        nnet_row_set(net, &tc, &tc0);
        printf("-- row_set tc=%d tc0=%d\n", tc, tc0);
    }
    void backward() { rc("backward", nnet_backward(net, ograd)); }
    // forward, backward, sgd, forward, backward
    void two_steps(int frames) {
        two_steps(frames, [this] { rc("sgd", nnet_sgd(net, 0.01f, 0.9f)); });
    }
    // the same with another parameter step between the two
    void two_steps(int frames, const std::function<void()> &step) {
        forward(frames);
        backward();
        step();
        forward(frames);
        backward();
    }
    void update() { rc("update", nnet_update(net, 0.01f, 0.9f, 2.0f, 1.0f)); }
    void sequences(const std::vector<int> &row0) { rc("set_sequences", nnet_set_sequences(net, row0.data(), (int)row0.size() - 1)); }
};

// a list getter's answer (nnet_dropout_layers and its like)
void list(const char *what, const KfNet *net, int (*get)(const KfNet *, int *, int)) {
    int idx[64];
    const int n = get(net, idx, 64);
    printf("-- %s -> %d", what, n);
    for (int i = 0; i < n && i < 64; ++i) printf(" %d", idx[i]);
    printf("\n");
}

KfNgOpts ng_defaults() {
    KfNgOpts o;
    kf_ng_default_opts(&o);
    return o;
}

// The modes whose combinations the host layer refuses (nnet_set_fp8, nnet_set_implicit_dz,
// nnet_set_row_subsampling, nnet_set_natural_gradient, nnet_bind_dp, nnet_set_dropout,
// nnet_set_bn_train). The data-parallel handle is opaque to the host layer, which only keeps
// it until a backward: no backward runs while this one is bound.
struct Mode {
    const char *name;
    int (*set)(KfNet *, bool on);
};
alignas(16) char g_fake_dp[16];
const Mode kFp8 = {"fp8", [](KfNet *n, bool on) { return nnet_set_fp8(n, on); }};
const Mode kIdz = {"implicit_dz", [](KfNet *n, bool on) { return nnet_set_implicit_dz(n, on); }};
const Mode kRsub = {"row_subsampling", [](KfNet *n, bool on) { return nnet_set_row_subsampling(n, on ? 3 : 0); }};
const Mode kNg = {"natgrad", [](KfNet *n, bool on) {
                      const KfNgOpts o = ng_defaults();
                      return nnet_set_natural_gradient(n, on ? &o : nullptr);
                  }};
const Mode kDp = {"dp", [](KfNet *n, bool on) { return nnet_bind_dp(n, on ? (KfDp *)g_fake_dp : nullptr, 1 << 20); }};
const Mode kDrop = {"dropout", [](KfNet *n, bool on) { return nnet_set_dropout(n, on, 7); }};
const Mode kBnt = {"bn_train", [](KfNet *n, bool on) { return nnet_set_bn_train(n, on); }};
const Mode kSa = {"spec_augment", [](KfNet *n, bool on) { return nnet_set_spec_augment(n, on, 7); }};

// a on, b on (refused when the two conflict), a off, b on again (never refused); all off at the end
void mode_pair(const std::string &cfg, const Mode &a, const Mode &b, const std::string &suffix = "") {
    scenario(std::string("modes/") + a.name + "_then_" + b.name + suffix);
    Run r(cfg, 150);
    rc((std::string(a.name) + " on").c_str(), a.set(r.net, true));
    rc((std::string(b.name) + " on").c_str(), b.set(r.net, true));
    rc((std::string(a.name) + " off").c_str(), a.set(r.net, false));
    rc((std::string(b.name) + " on").c_str(), b.set(r.net, true));
    rc((std::string(b.name) + " off").c_str(), b.set(r.net, false));
}

void env(const char *k, const char *v) {
    if (v) setenv(k, v, 1);
    else unsetenv(k);
}

void dp_plan(const KfNet *net, long long bucket_bytes) {
    int after[64];
    long long b[64], e[64];
    const int nb = nnet_dp_plan(net, bucket_bytes, 64, after, b, e);
    printf("-- dp_plan bucket_bytes=%lld -> %d", bucket_bytes, nb);
    for (int i = 0; i < nb; ++i) printf(" {after=%d %lld..%lld}", after[i], b[i], e[i]);
    printf("\n");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <configs dir>\n", argv[0]);
        return 2;
    }
    g_dir = argv[1];
    for (const char *k : {"KF_RSUB_CONV", "KF_DGRAD_WT"}) unsetenv(k);
    std::vector<std::string> cfgs;
    if (DIR *d = opendir(g_dir.c_str())) {
        while (dirent *e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > 8 && n.substr(n.size() - 8) == ".xconfig") cfgs.push_back(n);
        }
        closedir(d);
    }
    std::sort(cfgs.begin(), cfgs.end());
    const std::vector<std::string> two = {"tiny.xconfig", "cnn_tdnn_17f.xconfig"};

    for (const auto &c : cfgs) {
        scenario("config/" + c);
        Run r(c, 150);
        if (r.net) r.two_steps(150);
    }
    for (const auto &c : two)
        for (int on = 0; on <= 1; ++on) {
            scenario("wgrad_stream/" + c + "/" + (on ? "on" : "off"));
            Run r(c, 150);
            rc("set_wgrad_stream", nnet_set_wgrad_stream(r.net, on));
            r.two_steps(150);
        }
    for (const auto &c : two) {
        scenario("implicit_dz/" + c);
        Run r(c, 150);
        rc("set_implicit_dz", nnet_set_implicit_dz(r.net, 1));
        r.two_steps(150);
    }
    for (const auto &c : two)
        for (int aff = 0; aff <= 2; ++aff)
            for (int stall = 0; stall <= 1; ++stall) {
                scenario("debug_backward/" + c + "/aff" + std::to_string(aff) + (stall ? "/stall" : "/nostall"));
                Run r(c, 150);
                rc("debug_backward", nnet_debug_backward(r.net, aff, stall ? 100000 : 0));
                r.forward(150);
                r.backward();
            }
    for (const auto &c : two)
        for (int n : {1, 4}) {
            scenario("backward_n/" + c + "/" + std::to_string(n));
            Run r(c, 150);
            r.forward(150);
            rc("backward_n", nnet_backward_n(r.net, r.ograd, n));
        }
    // row subsampling: every residue of (T - 1) % 3, the compact conv on and off, one and two
    // streams, the transposed-weight input gradient on and off (both variables are read at
    // call time)
    for (const std::string &c : {std::string("tiny.xconfig"), std::string(kTinyS3), std::string("cnn_tdnn_17f.xconfig")})
        for (int i = 0; i < 3; ++i) {
            const int T = (c == "cnn_tdnn_17f.xconfig" ? 1498 : 150) + i;
            for (const char *conv : {(const char *)nullptr, "0"}) {
                // (only cnn_tdnn_17f's last conv can run on the compact rows: KF_RSUB_CONV=0
                // changes nothing for the tiny configs)
                if (conv && c != "cnn_tdnn_17f.xconfig") continue;
                for (int streams = 1; streams <= 2; ++streams)
                    for (const char *wt : {(const char *)nullptr, "0"}) {
                        scenario("row_subsampling/" + c + "/T" + std::to_string(T) + "/conv_" + (conv ? conv : "unset") +
                                 "/streams" + std::to_string(streams) + "/dgrad_wt_" + (wt ? wt : "unset"));
                        env("KF_RSUB_CONV", conv);
                        env("KF_DGRAD_WT", wt);
                        Run r(c, T);
                        rc("set_row_subsampling", nnet_set_row_subsampling(r.net, 3));
                        rc("set_wgrad_stream", nnet_set_wgrad_stream(r.net, streams == 2));
                        r.two_steps(T);
                    }
            }
        }
    env("KF_RSUB_CONV", nullptr);
    env("KF_DGRAD_WT", nullptr);
    {
        // tiny_s3: nt = 7, T = 101 gives tc0 = 34 < 4 * nt + 16: the step falls back to full rows
        scenario(std::string("row_subsampling/") + kTinyS3 + "/T101_below_guard");
        Run r(kTinyS3, 150);
        rc("set_row_subsampling", nnet_set_row_subsampling(r.net, 3));
        r.two_steps(101);
    }
    for (const std::string &c : {std::string("cnn_tdnn_17f_3072.xconfig"), std::string("tiny.xconfig")})
        for (int on = 1; on <= 2; ++on) {
            scenario("fp8/" + c + "/" + std::to_string(on));
            Run r(c, 150);
            rc("set_fp8", nnet_set_fp8(r.net, on));
            r.two_steps(150);
            (void)nnet_weight_buffer(r.net);
            rc("weights_changed", nnet_weights_changed(r.net));
            r.forward(150);
            r.backward();
        }
    for (const auto &c : two) {
        scenario("dp_plan/" + c);
        KfNet *net = nnet_create_layout(read_cfg(c).c_str(), 150);
        if (!net) return 3;
        dp_plan(net, 1 << 20);
        dp_plan(net, 8 << 20);
        nnet_free(net);
    }
    {
        scenario("negative/backward_before_forward");
        Run r("tiny.xconfig", 150);
        r.backward();
    }
    {
        scenario("negative/row_subsampling_stride2");
        Run r("tiny.xconfig", 150);
        rc("set_row_subsampling", nnet_set_row_subsampling(r.net, 2));
    }
    {
        scenario("negative/row_subsampling_tiny_att");
        Run r("tiny_att.xconfig", 150);
        rc("set_row_subsampling", nnet_set_row_subsampling(r.net, 3));
    }
    {
        scenario("negative/layout_only");
        KfNet *net = nnet_create_layout(read_cfg("tiny.xconfig").c_str(), 150);
        if (!net) return 3;
        std::vector<float> p((size_t)nnet_num_params(net), 0.f);
        rc("set_params", nnet_set_params(net, p.data()));
        rc("forward", nnet_forward(net, nullptr, 100));
        rc("backward", nnet_backward(net, nullptr));
        rc("sgd", nnet_sgd(net, 0.01f, 0.9f));
        rc("set_row_subsampling", nnet_set_row_subsampling(net, 3));
        rc("set_fp8", nnet_set_fp8(net, 1));
        nnet_free(net);
    }
    // ---- the Kaldi-style update ----
    {
        scenario("update/default");
        Run r("tiny.xconfig", 150);
        r.two_steps(150, [&] { r.update(); });
        r.update();
        float norms[64], scales[64], gn = 0, gs = 0;
        const int nc = nnet_num_components(r.net);
        printf("-- num_components %d\n", nc);
        rc("update_stats", nnet_update_stats(r.net, norms, scales, std::min(nc, 64), &gn, &gs));
    }
    {
        scenario("update/component_opts");
        Run r("tiny.xconfig", 150);
        r.forward(150);
        r.backward();
        r.update();
        rc("set_component_opts", nnet_set_component_opts(r.net, "tdnnf6.linear", 0.5f, 0.01f, 2.0f));
        r.forward(150);
        r.backward();
        r.update();  // (the component table again, not the segments)
        rc("update_stats", nnet_update_stats(r.net, nullptr, nullptr, 0, nullptr, nullptr));
    }
    // ---- the orthonormal constraint ----
    {
        scenario("orthonormal/tiny");
        Run r("tiny.xconfig", 150);
        list("orthonormal_components", r.net, nnet_orthonormal_components);
        rc("set_component_orthonormal", nnet_set_component_orthonormal(r.net, "tdnnf5.linear", 1.0f));
        rc("set_component_orthonormal", nnet_set_component_orthonormal(r.net, "tdnnf8.linear", 0.0f));
        list("orthonormal_components", r.net, nnet_orthonormal_components);
        r.two_steps(150, [&] {
            rc("sgd", nnet_sgd(r.net, 0.01f, 0.9f));
            rc("constrain_orthonormal", nnet_constrain_orthonormal(r.net));
        });
        rc("constrain_orthonormal", nnet_constrain_orthonormal(r.net));  // (no table is rebuilt)
        float sc[64], ratio[64], err[64];
        rc("orthonormal_stats", nnet_orthonormal_stats(r.net, sc, ratio, err, nnet_orthonormal_components(r.net, nullptr, 0)));
    }
    // ---- natural gradient: on, two steps and the read-backs, off again; one and two streams ----
    for (int streams = 1; streams <= 2; ++streams) {
        scenario("natgrad/tiny.xconfig/streams" + std::to_string(streams));
        Run r("tiny.xconfig", 150);
        const KfNgOpts o = ng_defaults();
        rc("set_natural_gradient", nnet_set_natural_gradient(r.net, &o));
        rc("set_wgrad_stream", nnet_set_wgrad_stream(r.net, streams == 2));
        r.two_steps(150);
        const int npre = nnet_natural_gradient_count(r.net);
        printf("-- natural_gradient_count %d\n", npre);
        std::vector<int> comp(npre), side(npre);
        std::vector<float> rep((size_t)npre * KF_NG_REPORT);
        rc("natural_gradient_stats", nnet_natural_gradient_stats(r.net, comp.data(), side.data(), rep.data(), npre));
        for (int i = 0; i < npre; ++i) printf("-- preconditioner %d: component %d side %d\n", i, comp[i], side[i]);
        int dim = 0, rank = 0;
        double rho = 0, t = 0;
        rc("natural_gradient_state", nnet_natural_gradient_state(r.net, 0, nullptr, nullptr, &dim, &rank, nullptr, nullptr, &rho, &t));
        printf("-- preconditioner 0: dim %d rank %d\n", dim, rank);
        rc("set_natural_gradient off", nnet_set_natural_gradient(r.net, nullptr));
        r.forward(150);
        r.backward();
    }
    // ---- per-sequence dropout: three unequal sequences, p = 0.3 ----
    // ("plain" never touches the switch: "off" must differ from it by its set_dropout line only)
    for (const std::string which : {"on", "off", "plain", "row_subsampling"}) {
        scenario("dropout/" + which);
        const bool rsub = which == "row_subsampling";
        Run r(rsub ? kTinyS3Drop : kTinyDrop, 150);
        list("dropout_layers", r.net, nnet_dropout_layers);
        r.sequences({0, 40, 90, 150});
        rc("set_dropout_proportion", nnet_set_dropout_proportion(r.net, nullptr, 0.3f));
        rc("set_dropout_proportion", nnet_set_dropout_proportion(r.net, "tdnnf7", 0.0f));
        float p = 0;
        rc("dropout_proportion", nnet_dropout_proportion(r.net, "tdnnf6", &p));
        printf("-- tdnnf6 p=%g\n", p);
        if (rsub) rc("set_row_subsampling", nnet_set_row_subsampling(r.net, 3));
        if (which != "plain") rc("set_dropout", nnet_set_dropout(r.net, which != "off", 1234));
        rc("set_dropout_step", nnet_set_dropout_step(r.net, 5));
        r.two_steps(150);
        printf("-- dropout_step %lld\n", nnet_dropout_step(r.net));
        std::vector<float> mask(3 * 256);
        int B = 0, dim = 0;
        rc("dropout_mask", nnet_dropout_mask(r.net, "tdnnf6", mask.data(), &B, &dim));
        printf("-- mask B=%d dim=%d\n", B, dim);
        rc("dropout_mask", nnet_dropout_mask(r.net, "tdnnf7", nullptr, &B, &dim));
    }
    // ---- SpecAugment: every config that has the layer, switch off and on, two sequences ----
    for (const char *c : {"specaug/cnn_tdnn_17f_kaldi_specaug.xconfig", "specaug/tiny_ivec_specaug.xconfig", kTinySa})
        for (int on = 0; on <= 1; ++on) {
            scenario(std::string(c) + (on ? "/on" : "/off"));
            Run r(c, 150);
            if (!r.net) continue;
            list("spec_augment_layers", r.net, nnet_spec_augment_layers);
            if (!r.is_ivec) r.sequences({0, 70, 150});  // (the ivector nets get theirs with the forward)
            double f = 0, z = 0;
            int m = 0;
            rc("spec_augment_opts", nnet_spec_augment_opts(r.net, "idct-spec-augment", &f, &z, &m));
            printf("-- opts f=%g z=%g m=%d\n", f, z, m);
            rc("set_spec_augment", nnet_set_spec_augment(r.net, on, 99));
            rc("set_spec_augment_step", nnet_set_spec_augment_step(r.net, 3));
            r.two_steps(150);
            printf("-- spec_augment_step %lld\n", nnet_spec_augment_step(r.net));
            std::vector<int32_t> rows(150);
            int T = 0;
            rc("spec_augment_rows", nnet_spec_augment_rows(r.net, "idct-spec-augment", rows.data(), &T));
            printf("-- rows T=%d\n", T);
            if (on) {  // no band and no time mask: the layer stays the alias of its input
                rc("set_spec_augment_opts", nnet_set_spec_augment_opts(r.net, "idct-spec-augment", 0.0, 0.0, 10));
                r.forward(150);
                rc("spec_augment_rows", nnet_spec_augment_rows(r.net, "idct-spec-augment", nullptr, &T));
            }
        }
    // ---- training-mode BatchNorm ----
    for (const std::string &c : {std::string("tiny.xconfig"), std::string(kTinyDrop), std::string("cnn_tdnn_17f.xconfig")}) {
        scenario("bn_train/" + c);
        Run r(c, 150);
        list("bn_train_layers", r.net, nnet_bn_train_layers);
        if (c == kTinyDrop) {
            r.sequences({0, 40, 90, 150});
            rc("set_dropout_proportion", nnet_set_dropout_proportion(r.net, nullptr, 0.3f));
            rc("set_dropout", nnet_set_dropout(r.net, 1, 1234));
        }
        rc("set_bn_train", nnet_set_bn_train(r.net, 1));
        r.two_steps(150);
        const char *layer = c == "cnn_tdnn_17f.xconfig" ? "tdnnf7" : "tdnnf6";
        std::vector<float> mean(4096), var(4096);
        std::vector<double> sum(4096), sumsq(4096);
        double count = -1;
        rc("bn_batch_stats", nnet_bn_batch_stats(r.net, layer, 0, mean.data(), var.data()));
        rc("bn_stats", nnet_bn_stats(r.net, layer, 0, &count, sum.data(), sumsq.data()));
        printf("-- count %g\n", count);
        printf("-- bn_commit -> %d\n", nnet_bn_commit(r.net));
        rc("bn_zero_stats", nnet_bn_zero_stats(r.net));
        rc("set_bn_train off", nnet_set_bn_train(r.net, 0));
        r.forward(150);
        r.backward();
    }
    // ---- the modes that cannot be combined: every pair in both orders ----
    {
        const Mode *pairs[][2] = {{&kFp8, &kNg}, {&kFp8, &kDrop}, {&kFp8, &kBnt}, {&kIdz, &kDrop}, {&kIdz, &kBnt},
                                  {&kRsub, &kBnt}, {&kNg, &kDp}, {&kDp, &kBnt}};
        for (const auto &pr : pairs) {
            mode_pair(kTinyS3Drop, *pr[0], *pr[1]);
            mode_pair(kTinyS3Drop, *pr[1], *pr[0]);
        }
        // SpecAugment x MXFP8: refused only where a layer would read the unmasked MXFP8 copy
        for (const char *c : {kTinySaMid, kTinySa}) {
            const std::string suffix = c == kTinySaMid ? "/conflict" : "/no_conflict";
            mode_pair(c, kFp8, kSa, suffix);
            mode_pair(c, kSa, kFp8, suffix);
        }
        // two modes that do combine
        mode_pair(kTinyS3Drop, kRsub, kDrop);
        // dropout on a net without a dropout layer is no mode: nothing conflicts with it
        mode_pair("tiny.xconfig", kFp8, kDrop, "/no_dropout_layer");
        // nnet_backward_n's refusals
        for (const Mode *m : {&kNg, &kDrop, &kBnt}) {
            scenario(std::string("modes/") + m->name + "_then_backward_n");
            Run r(kTinyS3Drop, 150);
            rc((std::string(m->name) + " on").c_str(), m->set(r.net, true));
            r.forward(150);
            rc("backward_n", nnet_backward_n(r.net, r.ograd, 2));
            rc((std::string(m->name) + " off").c_str(), m->set(r.net, false));
            r.forward(150);
            rc("backward_n", nnet_backward_n(r.net, r.ograd, 2));
        }
        // natural gradient x implicit dz: the setters accept it in either order, the backward refuses
        for (int order = 0; order <= 1; ++order) {
            const Mode &a = order ? kIdz : kNg, &b = order ? kNg : kIdz;
            scenario(std::string("modes/") + a.name + "_then_" + b.name);
            Run r("tiny.xconfig", 150);
            rc((std::string(a.name) + " on").c_str(), a.set(r.net, true));
            rc((std::string(b.name) + " on").c_str(), b.set(r.net, true));
            r.forward(150);
            r.backward();
        }
    }
    {
        scenario("negative/layout_only_new");
        KfNet *net = nnet_create_layout(read_cfg(kTinyDrop).c_str(), 150);
        if (!net) return 3;
        const KfNgOpts o = ng_defaults();
        const int seq[3] = {0, 70, 150};
        int n = 0;
        rc("update", nnet_update(net, 0.01f, 0.9f, 2.0f, 1.0f));
        rc("update_stats", nnet_update_stats(net, nullptr, nullptr, 0, nullptr, nullptr));
        rc("set_component_opts", nnet_set_component_opts(net, "tdnnf6.linear", 0.5f, 0.01f, 2.0f));
        rc("set_component_orthonormal", nnet_set_component_orthonormal(net, "tdnnf6.linear", 1.0f));
        rc("constrain_orthonormal", nnet_constrain_orthonormal(net));
        rc("orthonormal_stats", nnet_orthonormal_stats(net, nullptr, nullptr, nullptr, 0));
        rc("set_natural_gradient", nnet_set_natural_gradient(net, &o));
        rc("natural_gradient_stats", nnet_natural_gradient_stats(net, nullptr, nullptr, nullptr, 0));
        rc("natural_gradient_state", nnet_natural_gradient_state(net, 0, &n, &n, &n, &n, nullptr, nullptr, nullptr, nullptr));
        rc("set_sequences", nnet_set_sequences(net, seq, 2));
        rc("set_dropout_proportion", nnet_set_dropout_proportion(net, "tdnnf6", 0.3f));
        rc("set_dropout", nnet_set_dropout(net, 1, 1));
        rc("dropout_mask", nnet_dropout_mask(net, "tdnnf6", nullptr, &n, &n));
        rc("set_spec_augment", nnet_set_spec_augment(net, 1, 1));
        rc("spec_augment_rows", nnet_spec_augment_rows(net, "idct-spec-augment", nullptr, &n));
        rc("set_bn_train", nnet_set_bn_train(net, 1));
        rc("bn_batch_stats", nnet_bn_batch_stats(net, "tdnnf6", 0, nullptr, nullptr));
        rc("bn_stats", nnet_bn_stats(net, "tdnnf6", 0, nullptr, nullptr, nullptr));
        rc("bn_zero_stats", nnet_bn_zero_stats(net));
        printf("-- bn_commit -> %d: %s\n", nnet_bn_commit(net), nnet_last_error());
        rc("bind_dp", nnet_bind_dp(net, (KfDp *)g_fake_dp, 1 << 20));
        list("dropout_layers", net, nnet_dropout_layers);
        list("spec_augment_layers", net, nnet_spec_augment_layers);
        list("bn_train_layers", net, nnet_bn_train_layers);
        list("orthonormal_components", net, nnet_orthonormal_components);
        nnet_free(net);
    }
    {
        scenario("negative/dropout_no_layer");
        Run r("tiny.xconfig", 150);
        list("dropout_layers", r.net, nnet_dropout_layers);
        rc("set_dropout", nnet_set_dropout(r.net, 1, 1));
        rc("set_dropout_proportion", nnet_set_dropout_proportion(r.net, nullptr, 0.3f));
        rc("set_dropout_proportion", nnet_set_dropout_proportion(r.net, "tdnnf6", 0.3f));
        rc("set_dropout_proportion", nnet_set_dropout_proportion(r.net, "tdnnf99", 0.3f));
        float p = 0;
        rc("dropout_proportion", nnet_dropout_proportion(r.net, "tdnnf6", &p));
        printf("-- tdnnf6 p=%g\n", p);
        rc("dropout_proportion", nnet_dropout_proportion(r.net, "tdnnf99", &p));
        r.forward(150);
        rc("dropout_mask", nnet_dropout_mask(r.net, "tdnnf6", nullptr, nullptr, nullptr));
        rc("dropout_mask", nnet_dropout_mask(r.net, "tdnnf99", nullptr, nullptr, nullptr));
        rc("set_spec_augment", nnet_set_spec_augment(r.net, 1, 1));
        rc("spec_augment_opts", nnet_spec_augment_opts(r.net, "tdnnf6", nullptr, nullptr, nullptr));
        rc("spec_augment_rows", nnet_spec_augment_rows(r.net, "no-such-layer", nullptr, nullptr));
        rc("bn_batch_stats", nnet_bn_batch_stats(r.net, "tdnnf6", 0, nullptr, nullptr));
        rc("bn_stats", nnet_bn_stats(r.net, "prefinal-chain", 1, nullptr, nullptr, nullptr));
        rc("bn_stats", nnet_bn_stats(r.net, "cnn1", 0, nullptr, nullptr, nullptr));
    }
    {
        scenario("negative/ranges");
        Run r(kTinySa, 150);
        const int unordered[4] = {0, 90, 40, 150}, late[3] = {0, 70, 151}, first[3] = {1, 70, 150};
        KfNgOpts o = ng_defaults();
        o.update_period = 0;
        rc("set_dropout_step", nnet_set_dropout_step(r.net, -1));
        rc("set_dropout_step", nnet_set_dropout_step(r.net, 1ll << 32));
        rc("set_dropout_step", nnet_set_dropout_step(r.net, (1ll << 32) - 1));
        rc("set_spec_augment_step", nnet_set_spec_augment_step(r.net, -1));
        rc("set_spec_augment_step", nnet_set_spec_augment_step(r.net, 1ll << 32));
        rc("set_dropout_proportion", nnet_set_dropout_proportion(r.net, nullptr, 0.6f));
        rc("set_dropout_proportion", nnet_set_dropout_proportion(r.net, nullptr, -0.1f));
        rc("set_spec_augment_opts", nnet_set_spec_augment_opts(r.net, "idct-spec-augment", 1.5, 0.2, 10));
        rc("set_spec_augment_opts", nnet_set_spec_augment_opts(r.net, "idct-spec-augment", 0.5, 1.0, 10));
        rc("set_spec_augment_opts", nnet_set_spec_augment_opts(r.net, "idct-spec-augment", 0.5, 0.2, 0));
        rc("set_spec_augment_opts", nnet_set_spec_augment_opts(r.net, "cnn1", 0.5, 0.2, 10));
        rc("set_component_opts", nnet_set_component_opts(r.net, "tdnnf6.linear", -1.f, 0.f, 1.f));
        rc("set_component_opts", nnet_set_component_opts(r.net, "tdnnf6.linear", 1.f, 0.f, 0.f));
        rc("set_component_opts", nnet_set_component_opts(r.net, "no-such-component", 1.f, 0.f, 1.f));
        rc("set_component_orthonormal", nnet_set_component_orthonormal(r.net, "no-such-component", 1.f));
        rc("set_component_orthonormal", nnet_set_component_orthonormal(r.net, "tdnnf6.affine", 1.f));
        rc("set_component_orthonormal", nnet_set_component_orthonormal(r.net, "tdnnf6.linear", 1.f / 0.f));
        rc("set_component_orthonormal", nnet_set_component_orthonormal(r.net, "prefinal-l", 1.f));
        rc("set_sequences", nnet_set_sequences(r.net, unordered, 3));
        rc("set_sequences", nnet_set_sequences(r.net, late, 2));
        rc("set_sequences", nnet_set_sequences(r.net, first, 2));
        rc("set_sequences", nnet_set_sequences(r.net, nullptr, 0));
        rc("update", nnet_update(r.net, 0.01f, 0.9f, -1.0f, 1.0f));
        rc("update_stats", nnet_update_stats(r.net, nullptr, nullptr, 0, nullptr, nullptr));
        rc("orthonormal_stats", nnet_orthonormal_stats(r.net, nullptr, nullptr, nullptr, 0));
        rc("set_natural_gradient", nnet_set_natural_gradient(r.net, &o));
        rc("natural_gradient_stats", nnet_natural_gradient_stats(r.net, nullptr, nullptr, nullptr, 0));
        // sequences of another length than the forward's, with a per-sequence mask to draw
        const int seq[3] = {0, 70, 140};
        rc("set_sequences", nnet_set_sequences(r.net, seq, 2));
        rc("set_spec_augment", nnet_set_spec_augment(r.net, 1, 1));
        r.forward(150);
    }
    return 0;
}
