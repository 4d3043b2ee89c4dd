// prof.hip — optional per-launch HIP-event timing (kf_prof_*, include/kf_ops.h), used by
// bench.py to price the dominant kernel classes over the timed region on the stream they
// run on. Launch sites reach it through kf_prof.h only.
#include <vector>

#include "kf_prof.h"
#include "../../include/kf_ops.h"

namespace {
struct ProfRec {
    hipEvent_t a, b;
    KfProfRec r;
};
bool g_prof = false;
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_pool;
hipEvent_t prof_event() {
    if (!g_prof_pool.empty()) {
        hipEvent_t e = g_prof_pool.back();
        g_prof_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}
}  // namespace

bool kf_prof_take(const KfProfRec &rec, hipEvent_t *start, hipEvent_t *stop) {
    if (!g_prof) return false;
    ProfRec p{};
    *start = p.a = prof_event();
    *stop = p.b = prof_event();
    p.r = rec;
    g_prof_recs.push_back(p);
    return true;
}

int kf_prof_start(int cls, double work) { return kf_prof_start2(cls, work, 0.0); }
int kf_prof_start2(int cls, double flops, double bytes) {
    KfProfRec rec{};
    rec.cls = cls;
    rec.flops = flops;
    rec.bytes = bytes;
    hipEvent_t a, b;
    if (!kf_prof_take(rec, &a, &b)) return -1;
    hipEventRecord(a, kf_stream());
    return (int)g_prof_recs.size() - 1;
}
void kf_prof_stop(int idx) {
    if (idx < 0 || idx >= (int)g_prof_recs.size()) return;
    hipEventRecord(g_prof_recs[idx].b, kf_stream());
}

extern "C" void kf_prof_enable(int on) { g_prof = on != 0; }
// pre-create events for n timed launches' worth of records (two per launch), so that no
// hipEventCreate falls inside a timed region
extern "C" int kf_prof_reserve(int n) {
    while ((int)g_prof_pool.size() < 2 * n) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return -1;
        g_prof_pool.push_back(e);
    }
    return 0;
}
// sums per class since the last collect: count, milliseconds, flops, algorithmic bytes
extern "C" int kf_prof_collect2(int cls, long long *count, double *ms, double *flops, double *bytes) {
    kf_take_pending(__func__);
    long long c = 0;
    double t = 0, f = 0, by = 0;
    for (auto &p : g_prof_recs) {
        if (p.r.cls != cls) continue;
        hipEventSynchronize(p.b);
        kf_take_pending("kf_prof_collect2: hipEventSynchronize");
        float e = 0.f;
        hipEventElapsedTime(&e, p.a, p.b);
        kf_take_pending("kf_prof_collect2: hipEventElapsedTime");
        c++;
        t += e;
        f += p.r.flops;
        by += p.r.bytes;
    }
    if (count) *count = c;
    if (ms) *ms = t;
    if (flops) *flops = f;
    if (bytes) *bytes = by;
    return 0;
}
// every record since the last reset, in issue order (diagnostics): class, milliseconds,
// flops, GEMM shape and tile (0 for non-GEMM brackets); returns the count written
extern "C" int kf_prof_records(int max, int *cls, float *ms, double *flops, int *mnkt) {
    int i = 0;
    for (auto &p : g_prof_recs) {
        if (i >= max) break;
        hipEventSynchronize(p.b);
        float e = 0.f;
        hipEventElapsedTime(&e, p.a, p.b);
        cls[i] = p.r.cls;
        ms[i] = e;
        flops[i] = p.r.flops;
        mnkt[4 * i] = p.r.m;
        mnkt[4 * i + 1] = p.r.n;
        mnkt[4 * i + 2] = p.r.k;
        mnkt[4 * i + 3] = p.r.tile;
        ++i;
    }
    return i;
}
extern "C" int kf_prof_collect(int cls, long long *count, double *ms, double *flops) {
    return kf_prof_collect2(cls, count, ms, flops, nullptr);
}
// (no hipEventSynchronize here: a record of a stream destroyed since, e.g. a closed network's
// weight-gradient stream, made it fail with hipErrorStreamCaptureUnsupported; re-recording an
// event, also one still in flight, is what the next launch does anyway)
extern "C" void kf_prof_reset(void) {
    kf_take_pending(__func__);
    for (auto &p : g_prof_recs) {
        g_prof_pool.push_back(p.a);
        g_prof_pool.push_back(p.b);
    }
    g_prof_recs.clear();
}
