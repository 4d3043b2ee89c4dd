// conv_halo.hip — 3x3 (and strided) convolution forward and input gradient with the input
// halo resident in LDS: the kernel, its planner and its dispatch (gemm_host.h: conv_halo_try).
// The weight gradient's halo kernel is conv_wgrad.hip.
#include "gemm_kernel.h"

// ---------------------------------------------------------------------------
// Convolution with the input halo resident in LDS (forward, and the input gradient
// as a transposed convolution). The im2col GEMM (gemm_kernel) stages every tap's A rows
// through LDS separately, so a 3x3 conv moves each source element ~9x from L2;
// here a tile's source frames x heights x 64 channels land ONCE per channel chunk
// (one LDS-DMA sweep, zero rows for the time and height padding) and every tap's
// A fragment is read from that image at a per-tap row offset. The reduction runs
// chunk-major, tap-minor: K-step (c, p) = 64 channels of chunk c under tap p, so
// B (weights) still streams one 64-row slab per step through a 2-stage ring, and
// the halo of chunk c + 1 is issued in ntaps slices alongside, into the other of
// two halo buffers.
//
// Halo image: row R = f * hpos + pos holds source frame tbase + f and padded
// height shp = idx * hmul + par, where pos = par * hpe + idx (heights de-interleaved
// by parity when hmul = 2, so consecutive output heights read consecutive rows for
// every tap); 128 bytes per row. Row R's 16-byte chunk c sits at halo_off(R, c): 1 KiB
// piece R / 8, 16-byte slot (c + 2R) mod 16 of 256-byte block c / 2. A fragment read
// (16 lanes per ds_read_b128 group: eight rows at chunk c0, eight at c0 + 1, c0 even)
// then hits 16 distinct slots whenever its rows are consecutive halo rows, whatever the
// first row; with hpos = hout (mod 8) the rows of 16 consecutive output rows are
// consecutive modulo 8 across frame boundaries too (the host pads hpos when the LDS
// allows). The kc_off swizzle ((R >> 1) & 7) was 2-way conflicted for half of the
// starting rows and at every frame boundary (SQ_LDS_BANK_CONFLICT 0.30-0.40 of the
// LDS cycles).
// Output row m = (t, h) under tap p reads halo row
//     (t - tbase) * hpos + h + ctap[p]
// with ctap[p] = (dt_p - dtmin) * hpos + ((dh_p + pad) % hmul) * hpe + (dh_p + pad) / hmul.
// ---------------------------------------------------------------------------
// (halo_off: gemm_common.h, shared with splice_once.hip)
struct HaloArgs {
    const h16 *x;           // source [T x ...] rows of ld elements, heights of pw channels
    long long ld;
    int T, hout, hmul, hsrc, pw, pad, hpe, hpos, nf, dtmin;
    int ntaps, nch;         // taps, 64-channel chunks per tap
    int ts, toff;           // output frame t reads source frames ts * t + toff + dt (1 / 0: plain)
    int rows;               // halo rows per chunk image (nf * hpos)
    int npieces;            // 1 KiB LDS-DMA pieces per image (ceil(rows / 8))
    int slice;              // pieces issued per step (ceil(npieces / ntaps))
    int halo_bytes;         // per image, 1 KiB multiple
    int nbuf;               // halo images (2 when nch > 1)
    int ctap[KF_MAX_PARTS];
    int bshift[KF_MAX_PARTS];  // BROW: row shift of tap p's weight block (op_wrows)
    unsigned mhpos;            // ceil(2^32 / hpos): R / hpos = umulhi(R, mhpos)
    unsigned long long *trace;  // diagnostics (kf_halo_trace): block 300 wave 0 stamps, else null
};


// BROW: B is op_wrows' shifted weight rows (input gradient); the kernel then stages
// it as a plain 64-column operand whose base moves per step (scalar), instead of
// re-deriving every chunk's part offsets as the general stager would each step.
// ST: B ring stages. With ST > 2 the waits are counted (every wave knows how many
// loads it issued in each step: its share of that step's halo slice plus its B
// chunks), so ST - 2 weight stages stay in flight across each barrier.
template <int BM, int BN, int WM, int WN, bool BKC, int BMODE, bool BROW, int ST>
__global__ __launch_bounds__(64 * WM * WN, 1) void conv_halo_kernel(int M, int N, OpD B, KfEpilogue E,
                                                                    HaloArgs H, int n_mtiles,
                                                                    int n_ntiles) {
    constexpr int NW = WM * WN;
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 16, TN = WTN / 16;
    constexpr int B_STAGE = BN * BK * 2;
    // Waves 0 .. NWB-1 stage B (weights, L2), the others the next chunk's halo slices
    // (HBM). vmcnt is per wave and loads retire in order, so a B wave's per-step wait no
    // longer queues behind halo loads, and a halo wave waits only at a chunk start: the
    // slices get the whole chunk to land instead of one step.
    constexpr int NWB = NW / 2;
    using SB = Stager<BKC, BN, BMODE, NWB>;
    static_assert(SB::EVEN, "uniform B loads per B wave");
    static_assert(ST == 2, "the split-wave waits are written for a two-stage B ring");
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    char *bring = dsm + H.nbuf * H.halo_bytes;  // ST B stages after the halo images

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // XCD-aware tile order (as gemm_kernel): the N tiles of one M tile share an XCD
    const int ntiles = n_mtiles * n_ntiles;
    int tile = blockIdx.x;
    if (ntiles >= 8) {
        const int q = ntiles / 8, rmd = ntiles % 8, xcd = tile % 8, loc = tile / 8;
        tile = (xcd < rmd ? xcd * (q + 1) : rmd * (q + 1) + (xcd - rmd) * q) + loc;
    }
    const int mt = tile / n_ntiles, nt = tile - mt * n_ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int tbase = H.ts * (m0 / H.hout) + H.toff + H.dtmin;

    const bool bwave = wave < NWB;
    SB sb;
    if (bwave) sb.init(B, n0, wave, lane);
    const Rsrc rx = make_rsrc(H.x), rb = make_rsrc(B.base);
    const int K = H.ntaps * H.pw;

    // halo pieces [q0, q1) of chunk c into image `img`, strided over waves w0 .. w0+nw-1
    auto halo_issue = [&](int c, int img, int q0, int q1, int w0, int nw) {
        char *dst = dsm + img * H.halo_bytes;
        // lane l fills 16-byte position l of the piece: chunk kc, row 8q + r with
        // halo_off(R, kc) = 1024 q + 16 l (block kc / 2 = l / 16, slot (kc + 2r) mod 16 = l mod 16)
        const int slot = lane & 15, kc = 2 * (lane >> 4) + (slot & 1), r = ((slot - kc) & 15) >> 1;
        if (wave < w0) return;
        for (int q = q0 + wave - w0; q < q1; q += nw) {
            const int R = 8 * q + r;
            unsigned voff = BAD;
            if (R < H.rows) {
                // f = R / hpos by multiply-high (exact for every R < rows: host-checked);
                // hmul <= 2, so the parity half is one compare
                const int f = (int)__umulhi((unsigned)R, H.mhpos), pos = R - f * H.hpos;
                const int par = pos >= H.hpe ? 1 : 0, idx = pos - par * H.hpe;
                const int sh = idx * H.hmul + par - H.pad, t = tbase + f;
                if ((unsigned)t < (unsigned)H.T && (unsigned)sh < (unsigned)H.hsrc)
                    voff = (unsigned)(((long long)t * H.ld + (long long)sh * H.pw + c * BK + kc * 8) * 2);
            }
            lds_dma<16>(rx, dst + q * 1024, voff);
        }
    };

    // per-lane halo row of each 16-row group's row for tap 0 offset 0
    int rb0[TM];
    static_for<TM>([&](auto I) {
        const int r = wm * WTM + I * 16 + (lane & 15);
        const int m = min(m0 + r, M - 1);
        const int t = m / H.hout, h = m - t * H.hout;
        rb0[I] = (H.ts * t + H.toff - tbase + H.dtmin) * H.hpos + h;
    });

    float4v acc[TM][TN];
    static_for<TM>([&](auto I) {
        static_for<TN>([&](auto J) { acc[I][J] = float4v{0.f, 0.f, 0.f, 0.f}; });
    });

    const int steps = H.nch * H.ntaps;
    auto issue_b = [&](int st1, char *dst) {
        const int c1 = st1 / H.ntaps, p1 = st1 - c1 * H.ntaps;
        if (!bwave) return;
        if constexpr (BROW) {
            const h16 *bb = B.base + (long long)H.bshift[p1] * B.ld + c1 * BK;
            sb.issue(B, make_rsrc(bb), 0, BK, dst, wave, lane);
        } else {
            sb.issue(B, rb, p1 * H.pw + c1 * BK, K, dst, wave, lane);
        }
    };
    const bool tr = H.trace && blockIdx.x == 300 && tid == 0;
#define HALO_TP(slot) \
    if (tr && (slot) < 128) H.trace[slot] = wall_clock64();
    HALO_TP(0);
    const EpiPre epre = epi_params<BN, 64 * NW>(E, N, n0, tid);
    halo_issue(0, 0, 0, H.npieces, 0, NW);
    if (steps > 0) issue_b(0, bring);
    int sb_st = 0;  // B stage of step st
    for (int st = 0; st < steps; ++st) {
        const int c = st / H.ntaps, p = st - c * H.ntaps;
        // B waves: B(st), issued in step st - 1; halo waves: the whole halo of chunk c at
        // its first step (its slices were issued over chunk c - 1's steps)
        if (bwave || p == 0) wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        HALO_TP(1 + 2 * st);
        if (H.nbuf == 1 && c > 0 && p == 0) {
            // one halo image (two do not fit beside the B ring): every wave is past the
            // previous chunk's last fragment reads, so reload it in place and wait
            halo_issue(c, 0, 0, H.npieces, 0, NW);
            wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        // the halo slice first, then the B stage (the order the waits above count)
        if (H.nbuf > 1 && c + 1 < H.nch) {
            const int q0 = p * H.slice;
            halo_issue(c + 1, (c + 1) & 1, q0, min(H.npieces, q0 + H.slice), NWB, NW - NWB);
        }
        if (st + 1 < steps) issue_b(st + 1, bring + (sb_st ^ 1) * B_STAGE);
        const char *ta = dsm + (H.nbuf > 1 ? (c & 1) : 0) * H.halo_bytes;
        const char *tb = bring + sb_st * B_STAGE;
        sb_st = sb_st + 1 == ST ? 0 : sb_st + 1;
        const int ct = __builtin_amdgcn_readfirstlane(H.ctap[p]);
        static_for<BK / 32>([&](auto S) {
            constexpr int s = decltype(S)::value;
            half8 fa[TM], fb[TN];
            static_for<TM>([&](auto I) {
                const int R = rb0[I] + ct;
                fa[I] = *reinterpret_cast<const half8 *>(ta + halo_off(R, s * 4 + (lane >> 4)));
            });
            static_for<TN>([&](auto J) { fb[J] = load_frag<BKC, BN>(tb, wn * WTN + J * 16, s, lane); });
            static_for<TM>([&](auto I) {
                static_for<TN>([&](auto J) {
                    acc[I][J] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[I], fb[J], acc[I][J], 0, 0, 0);
                });
            });
        });
        __builtin_amdgcn_sched_barrier(0);
        HALO_TP(2 + 2 * st);
    }
    HALO_TP(126);
    fused_epilogue<BM, BN, WM, WN, BROW>(acc, dsm, E, M, N, m0, n0, tid, lane, wave, &epre);
    HALO_TP(127);
#undef HALO_TP
}

// ---------------------------------------------------------------------------
// conv_halo_kernel dispatch: A must be a conv im2col / col2im operand (k-contiguous,
// 64-channel parts, zero time padding, no edge rows, hdiv 1, hmul 1 or 2). Returns
// 1 when launched, 0 when not applicable (the caller runs the im2col GEMM), -1 on error.
// ---------------------------------------------------------------------------
static unsigned long long *g_halo_trace = nullptr;
static int g_halo_trace_at = -1, g_halo_launches = 0;
// diagnostics: stamp block 300 of the conv-halo launch number `at` (counted from this call)
extern "C" void kf_halo_trace(unsigned long long *buf, int at) {
    g_halo_trace = buf;
    g_halo_trace_at = at;
    g_halo_launches = 0;
}
// diagnostics: the geometry of the calling thread's last halo dispatch (kf_halo_debug_last)
static thread_local int g_halo_dbg[KF_HALO_DBG_N];
int *kf_halo_dbg_begin(int kind) {
    memset(g_halo_dbg, 0, sizeof g_halo_dbg);
    g_halo_dbg[0] = kind;
    return g_halo_dbg;
}
extern "C" int kf_halo_debug_last(int *out, int n) {
    const int m = std::min(std::max(n, 0), KF_HALO_DBG_N);
    for (int i = 0; out && i < m; ++i) out[i] = g_halo_dbg[i];
    return out ? m : 0;
}
template <int BM, int BN, int WM, int WN, bool BKC, int BMODE, bool BROW, int ST>
static int launch_halo(int M, int N, const OpD &B, const KfEpilogue &E, const HaloArgs &H0, size_t lds) {
    kf_take_pending(__func__);
    const int mt = (M + BM - 1) / BM, nt = (N + BN - 1) / BN;
    HaloArgs H = H0;
    H.trace = g_halo_trace && g_halo_launches++ == g_halo_trace_at ? g_halo_trace : nullptr;
    KfProfRec rec{};
    rec.cls = KF_PROF_HALO;
    rec.flops = 2.0 * M * N * (double)H.ntaps * H.pw;
    rec.m = M;
    rec.n = N;
    rec.k = H.ntaps * H.pw;
    rec.tile = BM * 10000 + BN;
    rec.bytes = (double)H.T * H.hsrc * H.pw * 2.0 + (double)H.ntaps * H.pw * N * 2.0 + epi_bytes(E, M, N);
    kf_launch(conv_halo_kernel<BM, BN, WM, WN, BKC, BMODE, BROW, ST>, dim3(mt * nt), dim3(64 * WM * WN), lds, &rec,
              M, N, B, E, H, mt, nt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kf_report_error("conv halo launch (M=%d N=%d): %s", M, N, hipGetErrorString(e));
        return -1;
    }
    return 1;
}

// What conv_halo_kernel would run for one product
struct HaloPlan {
    int BM_, BN_;  // tile
    bool brow;     // B is op_wrows' shifted weight rows (input gradient)
    HaloArgs H;
    size_t lds;    // dynamic LDS bytes
    OpD bp;        // B as the kernel stages it
};

// The plan for (M, N, K, a, b, E), or false when the halo kernel does not apply. Pure: no HIP
// call, nothing written but P and the calling thread's kf_halo_debug_last record.
static bool conv_halo_plan(int M, int N, int K, const OpD &a, const OpD &b, int bm, bool bkc,
                           const KfEpilogue &E, HaloPlan &P) {
    int *const dbg = kf_halo_dbg_begin(1);
    if (op_mode(a) != OP_GEN || !a.p64 || a.edges || a.tclamp || a.hshift ||
        a.hmul < 1 || a.hmul > 2 || a.hout < 2 || a.ncols != K || a.nparts * a.pw != K)
        return false;
    if (bkc ? bm != OP_GEN : bm != OP_SIMPLE) return false;
    if (E.edge_out) return false;  // the edge-row sum is the tiled kernel's (launch<> has its fallback)
    // shifted weight rows (op_wrows): every tap's block lies inside the matrix
    bool brow = bkc && b.hout == 1 && b.hmul == 0 && !b.hshift && !b.edges && !b.tclamp &&
                b.nparts == a.nparts && b.pw == a.pw;
    for (int p = 0; brow && p < b.nparts; ++p) brow = b.dt[p] >= 0 && b.dt[p] + b.nrows <= b.T;
    if (bkc && !brow) return false;
    if (E.row_group && !brow) return false;  // grouped rows: the input-gradient (BROW) kernels only
    P.brow = brow;
    P.bp = b;
    if (brow) {  // one 64-column chunk of a plain [nrows x ld] matrix, rebased per step
        OpD &bp = P.bp;
        bp.simple = 1;
        bp.nparts = 1;
        bp.ncols = BK;
        bp.pw = BK;
        bp.T = b.nrows;
        for (int p = 0; p < KF_MAX_PARTS; ++p) bp.dt[p] = bp.dh[p] = 0;
    }
    const TapGeom tg = tap_geometry(a);
    HaloArgs &H = P.H;
    memset(&H, 0, sizeof H);
    H.x = a.base;
    H.ld = a.ld;
    H.T = a.T;
    H.hout = a.hout;
    H.hmul = a.hmul;
    H.hsrc = a.hsrc;
    H.pw = a.pw;
    H.pad = tg.pad;
    const int hpe0 = tg.hpe;
    H.dtmin = tg.dtmin;
    H.ntaps = a.nparts;
    H.nch = a.pw / BK;
    // 32-bit source offsets: the largest byte offset the halo can form
    if (((long long)a.T * a.ld + (long long)a.hsrc * a.pw) * 2 >= (1LL << 32) - 64) return false;
    const int BN_ = P.BN_ = N <= 64 ? 64 : N <= 128 ? 128 : 256;
    // 256-row tiles, except 128-row tiles for the strided convs' per-residue input
    // gradients (3 or 6 taps; two workgroups per CU): cnn3 461 -> 332 and 588 -> 460 us,
    // cnn5 370 -> 317 and 536 -> 468 us
    const bool residue = a.nparts < 9;  // (B as shifted weight rows or a transposed copy)
    // time-strided rows (a.tmul > 1): a tile's output frames read tmul times the source
    // frames, so 128-row tiles keep the image in LDS
    const int BM_ = P.BM_ = residue || a.tmul > 1 ? 128 : 256;
    H.ts = a.tmul;
    H.toff = a.t0;
    H.nf = H.ts * ((BM_ - 1 + a.hout - 1) / a.hout) + 1 + (tg.dtmax - tg.dtmin);
    const int nw = BN_ == 64 ? 4 : 8;
    const size_t epi = 16 * BN_ + 32 * EpiMap<64>::LDT * 4 * nw;
    // LDS of a halo geometry: two images when there are several channel chunks, else one
    // (two too large, e.g. cnn5's stride-2 forward: 80 KB each beside a 64 KB B ring: one
    // image, reloaded between channel chunks)
    auto geometry = [&](int hpe, int &nbuf, int &halo_bytes) {
        halo_bytes = (H.nf * hpe * a.hmul + 7) / 8 * 1024;
        nbuf = H.nch > 1 ? 2 : 1;
        size_t l = std::max((size_t)nbuf * halo_bytes + 2 * BN_ * BK * 2, epi);
        if (l > 160 * 1024 && nbuf == 2) {
            nbuf = 1;
            l = std::max((size_t)halo_bytes + 2 * BN_ * BK * 2, epi);
        }
        return l;
    };
    int nb0, hb0;
    const size_t lds0 = geometry(hpe0, nb0, hb0);
    // hpos = hout (mod 8): conflict-free fragment reads across frame boundaries (halo_off),
    // taken when it keeps the image count and the workgroups per CU (80 KB: two)
    // (bounded: with hmul = 2 and an odd hout no pitch qualifies, so no pad is taken)
    int hpe = hpe0;
    while (hpe < hpe0 + 8 && (hpe * a.hmul - a.hout) % 8) ++hpe;
    const bool found8 = (hpe * a.hmul - a.hout) % 8 == 0;
    int nb1 = nb0, hb1 = hb0;
    const size_t lds1 = found8 ? geometry(hpe, nb1, hb1) : lds0;
    const bool pad8 = found8 && lds1 <= 160 * 1024 && nb1 == nb0 && (lds0 > 80 * 1024 || lds1 <= 80 * 1024);
    if (!pad8) hpe = hpe0;
    H.hpe = hpe;
    H.hpos = hpe * a.hmul;
    H.nbuf = pad8 ? nb1 : nb0;
    H.halo_bytes = pad8 ? hb1 : hb0;
    P.lds = pad8 ? lds1 : lds0;
    if (P.lds > 160 * 1024) return false;
    H.rows = H.nf * H.hpos;
    H.npieces = (H.rows + 7) / 8;
    H.mhpos = (unsigned)((0x100000000ULL + H.hpos - 1) / H.hpos);
    for (unsigned R = 0; R < (unsigned)(8 * H.npieces); ++R)
        if ((unsigned)(((unsigned long long)R * H.mhpos) >> 32) != R / (unsigned)H.hpos) return false;
    H.slice = (H.npieces + H.ntaps - 1) / H.ntaps;
    tap_rows(a, tg, H.hpe, H.ctap);
    for (int p = 0; p < a.nparts; ++p) H.bshift[p] = brow ? b.dt[p] : 0;
    const int v[] = {1, 1, BM_, BN_, brow, H.nch, H.nbuf, H.hpe, H.hpos, pad8, (M + BM_ - 1) / BM_,
                     (N + BN_ - 1) / BN_};
    std::copy(v, v + sizeof v / sizeof v[0], dbg);
    return true;
}

// the plan's instantiation
// (measured and dropped: a 4-stage weight ring at one workgroup per CU, cnn2 517 ->
// 884 us; 64-column tiles on two 128x64-tile waves, cnn2 529 -> 781 us)
template <bool BKC, bool BROW>
static int conv_halo_launch(int M, int N, const KfEpilogue &E, const HaloPlan &P) {
    const bool m128 = P.BM_ == 128;
    if (P.BN_ == 64)
        return m128 ? launch_halo<128, 64, 4, 1, BKC, OP_SIMPLE, BROW, 2>(M, N, P.bp, E, P.H, P.lds)
                    : launch_halo<256, 64, 4, 1, BKC, OP_SIMPLE, BROW, 2>(M, N, P.bp, E, P.H, P.lds);
    if (P.BN_ == 128)
        return m128 ? launch_halo<128, 128, 4, 2, BKC, OP_SIMPLE, BROW, 2>(M, N, P.bp, E, P.H, P.lds)
                    : launch_halo<256, 128, 4, 2, BKC, OP_SIMPLE, BROW, 2>(M, N, P.bp, E, P.H, P.lds);
    return m128 ? launch_halo<128, 256, 2, 4, BKC, OP_SIMPLE, BROW, 2>(M, N, P.bp, E, P.H, P.lds)
                : launch_halo<256, 256, 2, 4, BKC, OP_SIMPLE, BROW, 2>(M, N, P.bp, E, P.H, P.lds);
}

int conv_halo_try(int M, int N, int K, const OpD &a, const OpD &b, int bm, bool bkc, const KfEpilogue &E) {
    HaloPlan P;
    if (!conv_halo_plan(M, N, K, a, b, bm, bkc, E, P)) return 0;
    return P.brow ? conv_halo_launch<true, true>(M, N, E, P) : conv_halo_launch<false, false>(M, N, E, P);
}
