// loss_scale.hip — the dynamic loss scale of the fp16 train step, kept on the device
// (include/kf_ops.h kf_loss_scale_*).
//
// The state is one small block of device memory (loss_scale_state.h). Per step, on the current
// stream, with no host round trip and no atomics:
//   k_ls_check    over the update's segment table, cut as k_upd_velocity cuts it (one workgroup
//                 per KF_UPD_CHUNK chunk of one segment, 16-byte vector body, scalar head and
//                 tail): flag[b] = the chunk holds a non-finite element. What no segment covers
//                 (the alignment padding between tensors) is not read. HBM-bound: 4 bytes per
//                 parameter, one read of the gradient buffer.
//   k_ls_advance  one workgroup folds the flags (an OR: the order does not matter) and one lane
//                 advances the state in plain C++: inv_used = 1 / scale latched first, then skip,
//                 scale, since and the counters.
// The update kernels (update.hip, layers.hip k_sgd_flat_scaled) then load skip and inv_used
// block-uniformly. k_ls_init / k_ls_set are one-thread launches, stream-ordered like the rest.
#include "upd_chunk.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFoldThreads = 1024;
static_assert(KF_UPD_CHUNK % (4 * kThreads) == 0, "a chunk is whole float4 rounds of the workgroup");

// inf or NaN: the exponent field is all ones
__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(kThreads) void k_ls_check(const float *__restrict__ g, long long n,
                                                       const KfUpdSegment *__restrict__ segs, int nseg, int ncomp,
                                                       int *__restrict__ flag) {
    long long cb, ce, a0, a1;
    int c;
    bool bad = false;
    if (upd_chunk(segs, nseg, ncomp, n, blockIdx.x, cb, ce, c)) {  // the same in every thread
        upd_split(cb, ce, a0, a1);
        for (long long i = a0 + 4 * threadIdx.x; i < a1; i += 4 * kThreads) {
            const float4v gv = *reinterpret_cast<const float4v *>(g + i);
            bad = bad || non_finite(gv[0]) || non_finite(gv[1]) || non_finite(gv[2]) || non_finite(gv[3]);
        }
        const long long i = upd_scalar(cb, ce, a0, a1, threadIdx.x);
        if (i >= 0) bad = bad || non_finite(g[i]);
    }
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) flag[blockIdx.x] = any;  // every workgroup of the grid writes its flag
}

__device__ __forceinline__ float ls_clamp(float s, float lo, float hi) { return fminf(fmaxf(s, lo), hi); }

__global__ __launch_bounds__(kFoldThreads) void k_ls_advance(const int *__restrict__ flag, int nflag,
                                                             KfLossScaleState *__restrict__ st) {
    int bad = 0;
    for (int i = threadIdx.x; i < nflag; i += kFoldThreads) bad |= flag[i];
    const int overflow = __syncthreads_or(bad) ? 1 : 0;
    if (threadIdx.x != 0) return;
    KfLossScaleState s = *st;
    s.inv_used = 1.0f / s.scale;  // the scale this step's objective read, before the state moves
    s.skip = overflow;
    s.last_overflow = overflow;
    s.steps += 1;
    if (overflow) {
        s.skipped += 1;
        s.scale = fmaxf(s.min_scale, s.scale * s.backoff);
        s.since = 0;
    } else if (++s.since >= s.growth_interval) {
        s.scale = fminf(s.max_scale, s.scale * s.growth);
        s.since = 0;
    }
    *st = s;
}

__global__ void k_ls_init(KfLossScaleState *st, KfLossScaleOpts o) {
    if (blockIdx.x || threadIdx.x) return;
    KfLossScaleState s;
    s.scale = ls_clamp(o.init_scale, o.min_scale, o.max_scale);
    s.inv_used = 1.0f / s.scale;
    s.since = 0;
    s.skip = 0;
    s.steps = 0;
    s.skipped = 0;
    s.last_overflow = 0;
    s.growth_interval = o.growth_interval;
    s.growth = o.growth;
    s.backoff = o.backoff;
    s.min_scale = o.min_scale;
    s.max_scale = o.max_scale;
    *st = s;
}

__global__ void k_ls_set(KfLossScaleState *st, float scale) {
    if (blockIdx.x || threadIdx.x) return;
    st->scale = ls_clamp(scale, st->min_scale, st->max_scale);
    st->since = 0;
}

bool launched(const char *fn) {
    if (hipGetLastError() == hipSuccess) return true;
    kf_report_error("%s: launch failed", fn);
    return false;
}

}  // namespace

extern "C" void kf_loss_scale_default_opts(KfLossScaleOpts *o) {
    if (o) *o = KfLossScaleOpts{65536.f, 2.f, 0.5f, 2000, 1.f, 65536.f};
}

extern "C" long long kf_loss_scale_state_bytes(void) { return (long long)sizeof(KfLossScaleState); }

extern "C" long long kf_loss_scale_scratch_bytes(long long n, int nseg) {
    if (n < 0 || nseg < 0) return -1;
    return upd_grid(n, nseg) * 4;
}

extern "C" int kf_loss_scale_init(void *state, const KfLossScaleOpts *o) {
    kf_take_pending(__func__);
    if (!state || (uintptr_t)state % 16 || !o) {
        kf_report_error("kf_loss_scale_init: null or misaligned state (16 bytes), or null options");
        return -1;
    }
    // (written so that a NaN fails each test)
    if (!(o->min_scale > 0.f) || !(o->max_scale >= o->min_scale) || !(o->max_scale <= 3.0e38f) ||
        !(o->init_scale > 0.f) || !(o->growth >= 1.f) || !(o->growth <= 3.0e38f) || !(o->backoff > 0.f) ||
        !(o->backoff <= 1.f) || o->growth_interval < 1) {
        kf_report_error("kf_loss_scale_init: bad options (init_scale %g > 0, growth %g >= 1, 0 < backoff %g <= 1, "
                        "growth_interval %d >= 1, 0 < min_scale %g <= max_scale %g, all finite)",
                        (double)o->init_scale, (double)o->growth, (double)o->backoff, o->growth_interval,
                        (double)o->min_scale, (double)o->max_scale);
        return -1;
    }
    k_ls_init<<<1, 1, 0, kf_stream()>>>((KfLossScaleState *)state, *o);
    return launched(__func__) ? 0 : -1;
}

extern "C" int kf_loss_scale_set_scale(void *state, float scale) {
    kf_take_pending(__func__);
    if (!state || !(scale > 0.f)) {
        kf_report_error("kf_loss_scale_set_scale: null state, or scale %g not above 0", (double)scale);
        return -1;
    }
    k_ls_set<<<1, 1, 0, kf_stream()>>>((KfLossScaleState *)state, scale);
    return launched(__func__) ? 0 : -1;
}

extern "C" int kf_loss_scale_check(void *state, const float *g, long long n, const KfUpdSegment *segments, int nseg,
                                   int ncomp, void *scratch) {
    kf_take_pending(__func__);
    if (n < 0 || nseg < 0 || ncomp < 0) {
        kf_report_error("kf_loss_scale_check: bad arguments (n %lld, %d segments, %d components)", n, nseg, ncomp);
        return -1;
    }
    const long long grid = upd_grid(n, nseg);
    if (!state || !scratch || (uintptr_t)scratch % 4 || grid > 0x7fffffffll ||
        (n && nseg && (!g || !segments || (uintptr_t)g % 16))) {
        kf_report_error("kf_loss_scale_check: null or misaligned buffer (g 16 bytes, scratch 4), or more than 2^31 "
                        "workgroups");
        return -1;
    }
    // an empty table: nothing to check, the step counts as clean (grid >= 0 flags, none set)
    const int nflag = n && nseg && ncomp ? (int)grid : 0;
    if (nflag)
        k_ls_check<<<(unsigned)nflag, kThreads, 0, kf_stream()>>>(g, n, segments, nseg, ncomp, (int *)scratch);
    k_ls_advance<<<1, kFoldThreads, 0, kf_stream()>>>((const int *)scratch, nflag, (KfLossScaleState *)state);
    return launched(__func__) ? 0 : -1;
}

extern "C" int kf_loss_scale_read(const void *state, float *scale, int *since, long long *steps, long long *skipped,
                                  int *last_overflow) {
    kf_take_pending(__func__);
    if (!state) {
        kf_report_error("kf_loss_scale_read: null state");
        return -1;
    }
    KfLossScaleState s;
    hipStream_t st = kf_stream();
    if (hipMemcpyAsync(&s, state, sizeof s, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        kf_take_pending("kf_loss_scale_read copy");
        kf_report_error("kf_loss_scale_read: copy failed");
        return -1;
    }
    if (scale) *scale = s.scale;
    if (since) *since = s.since;
    if (steps) *steps = s.steps;
    if (skipped) *skipped = s.skipped;
    if (last_overflow) *last_overflow = s.last_overflow;
    return 0;
}
