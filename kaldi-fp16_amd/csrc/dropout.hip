// dropout.hip — per-sequence dropout masks of the TDNN-F layers (kf_ops.h kf_dropout_masks /
// kf_row_seg): Kaldi's GeneralDropoutComponent with continuous = true,
// time-period = 0 and block-dim = dim, one random scale per (sequence, column) shared by all
// frames of the sequence. The masks of every layer of a forward come from one launch of a
// counter-based generator (Philox4x32-10, Salmon et al., SC'11), so nothing random lives on the
// device and the same (seed, step) gives the same masks whatever the launch geometry. The
// fused GEMM epilogue (gemm_kernel.h, KfEpilogue.drop) applies them.
#include "kf_common.h"
#include "../../include/kf_ops.h"

namespace {

constexpr int kThreads = 256;

struct DropTable {
    KfDropLayer l[KF_DROP_MAX];
};

__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0;
    c[1] = n1;
    c[2] = n2;
    c[3] = n3;
}

// thread = one Philox block = columns 4j .. 4j + 3 of row b of layer blockIdx.z's mask
__global__ __launch_bounds__(kThreads) void k_dropout_masks(DropTable t, int B, unsigned k0, unsigned k1, unsigned step) {
    const KfDropLayer L = t.l[blockIdx.z];
    const int j = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    if (4 * j >= L.dim || b >= B) return;
    unsigned c[4] = {step, (unsigned)L.ordinal, (unsigned)b, (unsigned)j};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const float a = 4.f * L.p, o = 1.f - 2.f * L.p;
    float4v m;
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = fmaf(a, (float)(c[e] >> 8) * 0x1p-24f, o);
    *reinterpret_cast<float4v *>(L.mask + (long long)b * L.ld + 4 * j) = m;
}

// source row of GEMM row r (kf_gather_rows' compact-row rule when tc > 0), then its sequence
__global__ __launch_bounds__(kThreads) void k_row_seg(int *row_seg, const int *seq_off, int B, int T, int tc0, int tc) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= (tc > 0 ? tc : T)) return;
    const int t = tc <= 0 ? r : r < tc0 ? 3 * r : (T - 1) - 3 * (tc - 1 - r);
    int lo = 0, hi = B - 1;  // the last b with seq_off[b] <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seq_off[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    row_seg[r] = lo;
}

}  // namespace

extern "C" int kf_dropout_masks(int n, const KfDropLayer *layers, int B, unsigned long long seed, long long step) {
    kf_take_pending(__func__);
    if (n < 0 || (n > 0 && !layers) || B <= 0 || step < 0 || step > 0xFFFFFFFFll) {
        kf_report_error("kf_dropout_masks: bad arguments (n=%d B=%d step=%lld: 0 <= step < 2^32)", n, B, step);
        return -1;
    }
    for (int i = 0; i < n; ++i) {
        const KfDropLayer &l = layers[i];
        if (!(l.p >= 0.f && l.p <= 0.5f) || l.dim <= 0 || l.dim % 4 || l.ld < l.dim || l.ld % 4 || !l.mask ||
            ((uintptr_t)l.mask & 15) || l.ordinal < 0) {
            kf_report_error("kf_dropout_masks: layer %d needs 0 <= p <= 0.5, dim %% 4 == 0, ld >= dim, ld %% 4 == 0 and "
                            "a 16-byte aligned mask (p=%g dim=%d ld=%lld)", i, (double)l.p, l.dim, l.ld);
            return -1;
        }
    }
    // one launch per KF_DROP_MAX layers with p > 0 (p = 0: the identity, nothing is written)
    for (int i = 0; i < n;) {
        DropTable t;
        int cnt = 0, maxdim = 0;
        for (; i < n && cnt < KF_DROP_MAX; ++i) {
            if (layers[i].p == 0.f) continue;
            t.l[cnt++] = layers[i];
            maxdim = layers[i].dim > maxdim ? layers[i].dim : maxdim;
        }
        if (!cnt) break;
        const dim3 grid((unsigned)((maxdim / 4 + kThreads - 1) / kThreads), (unsigned)B, (unsigned)cnt);
        if (B > 65535) {
            kf_report_error("kf_dropout_masks: more than 65535 sequences (B=%d)", B);
            return -1;
        }
        k_dropout_masks<<<grid, kThreads, 0, kf_stream()>>>(t, B, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)step);
    }
    return hipGetLastError() == hipSuccess ? 0 : (kf_report_error("kf_dropout_masks: launch failed"), -1);
}

extern "C" int kf_row_seg(int32_t *row_seg, const int *dev_seq_off, int B, int T, int tc0, int tc) {
    kf_take_pending(__func__);
    if (!row_seg || T <= 0 || B < 0 || (B > 1 && !dev_seq_off) || tc < 0 || tc0 < 0 || tc0 > tc ||
        (tc > 0 && (3LL * (tc0 - 1) > T - 1 || (long long)(T - 1) - 3LL * (tc - tc0 - 1) < 0 || tc > tc0 + T))) {
        kf_report_error("kf_row_seg: bad arguments (B=%d T=%d tc0=%d tc=%d)", B, T, tc0, tc);
        return -1;
    }
    const int rows = tc > 0 ? tc : T;
    if (B <= 1) {  // one sequence
        if (hipMemsetAsync(row_seg, 0, (size_t)rows * 4, kf_stream()) != hipSuccess) {
            kf_report_error("kf_row_seg: memset failed");
            return -1;
        }
        return 0;
    }
    k_row_seg<<<(unsigned)((rows + kThreads - 1) / kThreads), kThreads, 0, kf_stream()>>>(row_seg, dev_seq_off, B, T, tc0, tc);
    return hipGetLastError() == hipSuccess ? 0 : (kf_report_error("kf_row_seg: launch failed"), -1);
}
