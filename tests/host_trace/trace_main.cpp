// trace_main.cpp — drives the host layer (nnet_*) over the stub backend and prints, per
// scenario, the C-ABI calls it made (stub_backend.cpp) and the error texts of the negative
// cases. usage: host_trace <configs dir>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <dirent.h>
#include <fstream>
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

std::string read_cfg(const std::string &name) {
    if (name == kTinyS3) {
        std::string t = read_cfg("tiny.xconfig");
        const std::string from = "time-stride=1", to = "time-stride=3";
        const size_t at = t.find(from);
        if (at == std::string::npos) exit(2);
        return t.replace(at, from.size(), to);
    }
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
        forward(frames);
        backward();
        rc("sgd", nnet_sgd(net, 0.01f, 0.9f));
        forward(frames);
        backward();
    }
};

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
    return 0;
}
