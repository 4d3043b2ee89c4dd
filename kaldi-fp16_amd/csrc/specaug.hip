// specaug.hip — SpecAugment masks of the spec-augment-layer (kf_ops.h kf_specaug_rows /
// kf_specaug_apply): Kaldi's GeneralDropoutComponent with
// specaugment-max-proportion (one zeroed frequency band per sequence) followed by its
// SpecAugmentTimeMaskComponent (alternating kept and zeroed runs of frames). Every draw comes
// from dropout.hip's counter-based Philox4x32-10 keyed by (seed, step), so nothing random lives
// on the device and a (seed, step) replays exactly. kf_specaug_rows writes one int32 per frame
// (the row's band, or -1 for a zeroed frame); kf_specaug_apply is the select that reads it.
#include "kf_common.h"
#include "../../include/kf_ops.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0;
    c[1] = n1;
    c[2] = n2;
    c[3] = n3;
}

// X(b, kind, i): word i % 4 of the block with counter {step, 0x80000000 | (2k + kind), b, i / 4}
__device__ __forceinline__ unsigned draw(unsigned step, unsigned stream, unsigned b, unsigned i, unsigned k0, unsigned k1) {
    unsigned c[4] = {step, stream, b, i >> 2};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const unsigned w = i & 3;
    return w == 0 ? c[0] : w == 1 ? c[1] : w == 2 ? c[2] : c[3];
}

// an integer in [0, n): (u24(x) n) >> 24, exact in 64 bits
__device__ __forceinline__ unsigned randint(unsigned x, unsigned n) {
    return (unsigned)(((unsigned long long)(x >> 8) * n) >> 24);
}

// wave = one sequence. The band first; then, pass by pass, lane l draws the length of region
// 64 p + l, an inclusive prefix sum over the wave (saturating at the sequence's length, so it
// stays in 32 bits whatever max_kept is) gives the regions' ends, and the wave writes the
// frames the pass covers, 64 at a time, each lane finding its frame's region by bisection
// over the lanes' ends.
__global__ __launch_bounds__(kThreads) void k_specaug_rows(int32_t *row_band, const int *seq_off, int B, int T, int dim,
                                                          int max_bins, float z, unsigned max_zeroed, unsigned max_kept,
                                                          unsigned ordinal, unsigned k0, unsigned k1, unsigned step) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (b >= B) return;
    int s0 = 0, s1 = T;
    if (seq_off) {  // (clamped: a bad offset table writes nothing outside [0, T))
        s0 = min(max(seq_off[b], 0), T);
        s1 = min(max(seq_off[b + 1], s0), T);
    }
    const unsigned len = (unsigned)(s1 - s0);
    const unsigned sf = 0x80000000u | (2u * ordinal), st = sf | 1u;
    const unsigned count = randint(draw(step, sf, (unsigned)b, 0, k0, k1), (unsigned)max_bins + 1u);
    const unsigned start = randint(draw(step, sf, (unsigned)b, 1, k0, k1), (unsigned)dim - count + 1u);
    const int32_t band = (int32_t)(start | count << 16);
    int32_t *out = row_band + s0;
    if (!(z > 0.f)) {
        for (unsigned t = lane; t < len; t += 64) out[t] = band;
        return;
    }
    const unsigned first = (float)(draw(step, st, (unsigned)b, 0, k0, k1) >> 8) * 0x1p-24f < z ? 1u : 0u;
    unsigned carry = 0;  // frames the passes before covered
    for (unsigned pass = 0; carry < len; ++pass) {
        const unsigned r = 64u * pass + lane;
        const unsigned zeroed = first ^ (r & 1u);
        const unsigned l = 1u + randint(draw(step, st, (unsigned)b, 1u + r, k0, k1), zeroed ? max_zeroed : max_kept);
        unsigned end = min(l, len);  // inclusive prefix sum, saturating at len (< 2^31)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(end, d, 64);
            if (lane >= d) end = min(end + o, len);
        }
        const unsigned total = min(__shfl(end, 63, 64), len - carry);
        for (unsigned base = 0; base < total; base += 64) {
            const unsigned off = base + lane;  // frame carry + off lies in the first lane whose end > off
            int lo = 0, hi = 63;
#pragma unroll
            for (int it = 0; it < 6; ++it) {
                const int mid = (lo + hi) >> 1;
                if (__shfl(end, mid, 64) > off) hi = mid;
                else lo = mid + 1;
            }
            if (off < total) out[carry + off] = (first ^ ((unsigned)lo & 1u)) ? -1 : band;
        }
        carry += total;
    }
}

typedef unsigned short ushort8v __attribute__((ext_vector_type(8)));

// thread = 8 columns of one row, 16 bytes in and out
__global__ __launch_bounds__(kThreads) void k_specaug_apply_v8(const unsigned short *x, long long ldx, unsigned short *y, long long ldy,
                                                              long long rows, int dim8, const int32_t *row_band) {
    const long long n = rows * dim8, S = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += S) {
        const long long r = i / dim8;
        const int c = (int)(i - r * dim8) * 8;
        const int32_t rb = row_band[r];
        ushort8v v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (rb != -1) {
            const int b0 = rb & 0xFFFF, b1 = b0 + (rb >> 16);
            v = *reinterpret_cast<const ushort8v *>(x + r * ldx + c);
            if (c < b1 && c + 8 > b0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (c + e >= b0 && c + e < b1) ? (unsigned short)0 : v[e];
            }
        }
        *reinterpret_cast<ushort8v *>(y + r * ldy + c) = v;
    }
}

__global__ __launch_bounds__(kThreads) void k_specaug_apply_s(const unsigned short *x, long long ldx, unsigned short *y, long long ldy,
                                                             long long rows, int dim, const int32_t *row_band) {
    const long long n = rows * dim, S = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += S) {
        const long long r = i / dim;
        const int c = (int)(i - r * dim);
        const int32_t rb = row_band[r];
        const int b0 = rb & 0xFFFF, b1 = b0 + (rb >> 16);
        const bool zero = rb == -1 || (c >= b0 && c < b1);
        y[r * ldy + c] = zero ? (unsigned short)0 : x[r * ldx + c];
    }
}

}  // namespace

extern "C" int kf_specaug_rows(int32_t *row_band, const int *dev_seq_off, int B, int T, int dim, int max_bins, float z,
                               int max_zeroed, int max_kept, unsigned ordinal, unsigned long long seed, long long step) {
    kf_take_pending(__func__);
    if (!row_band || T <= 0 || B < 0 || dim <= 0 || dim > 32767 || max_bins < 0 || max_bins > dim || !(z >= 0.f && z < 1.f) ||
        max_zeroed < 1 || max_kept < 1 || ordinal > 0x3FFFFFFFu || step < 0 || step > 0xFFFFFFFFll) {
        kf_report_error("kf_specaug_rows: bad arguments (B=%d T=%d dim=%d max_bins=%d z=%g max_zeroed=%d max_kept=%d "
                        "ordinal=%u step=%lld: 0 < dim <= 32767, 0 <= max_bins <= dim, 0 <= z < 1, 0 <= step < 2^32)",
                        B, T, dim, max_bins, (double)z, max_zeroed, max_kept, ordinal, step);
        return -1;
    }
    const bool one = B <= 1 || !dev_seq_off;  // one sequence [0, T)
    const int nb = one ? 1 : B;
    k_specaug_rows<<<(unsigned)((nb + kWaves - 1) / kWaves), kThreads, 0, kf_stream()>>>(
        row_band, one ? nullptr : dev_seq_off, nb, T, dim, max_bins, z, (unsigned)max_zeroed, (unsigned)max_kept, ordinal,
        (unsigned)seed, (unsigned)(seed >> 32), (unsigned)step);
    return hipGetLastError() == hipSuccess ? 0 : (kf_report_error("kf_specaug_rows: launch failed"), -1);
}

extern "C" int kf_specaug_apply(const void *x, long long ldx, void *y, long long ldy, long long rows, int dim,
                                const int32_t *row_band) {
    kf_take_pending(__func__);
    if (!x || !y || !row_band || rows < 0 || dim < 1 || dim > 32767 || ldx < dim || ldy < dim) {
        kf_report_error("kf_specaug_apply: bad arguments (rows=%lld dim=%d ldx=%lld ldy=%lld: 1 <= dim <= 32767, ld >= dim)",
                        rows, dim, ldx, ldy);
        return -1;
    }
    if (rows == 0) return 0;
    const bool vec = dim % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && !(((uintptr_t)x | (uintptr_t)y) & 15);
    if (vec)
        k_specaug_apply_v8<<<kf_blocks(rows * (dim / 8), kThreads, 1 << 16), kThreads, 0, kf_stream()>>>(
            (const unsigned short *)x, ldx, (unsigned short *)y, ldy, rows, dim / 8, row_band);
    else
        k_specaug_apply_s<<<kf_blocks(rows * dim, kThreads, 1 << 16), kThreads, 0, kf_stream()>>>(
            (const unsigned short *)x, ldx, (unsigned short *)y, ldy, rows, dim, row_band);
    return hipGetLastError() == hipSuccess ? 0 : (kf_report_error("kf_specaug_apply: launch failed"), -1);
}
