// splice_once.hip — the long-K N = bottleneck products on a two-part spliced A operand with
// the source rows resident in LDS: the kernel, its planner and its dispatch (gemm_host.h:
// splice_once_try). The TDNN-F linear forward ([x(t-s) | x(t)]) and affine input gradient
// ([dz(t) | dz(t-s)]) at the row-subsampled step's row count.
#include "gemm_kernel.h"

// ---------------------------------------------------------------------------
// gemm_kernel with the K-step interleave (kil) alternates (part 0, chunk c) and (part 1,
// chunk c): the same 64-column chunk of the same source rows, shifted by the splice offset,
// is fetched into LDS twice and waited for twice, each behind its own barrier. Here, as in
// the conv halo kernel, a 128-row tile's source rows m0 + min(dt) .. m0 + 127 + max(dt) of
// chunk c land ONCE (one LDS-DMA sweep) and both parts' A fragments are read from that image
// at a per-lane row: the reduction still runs chunk-major, part 0 then part 1, sub-steps in
// K order, the order kofs() gives with kil on, so every accumulator sees the same MFMAs on
// the same operands in the same order and the outputs are bit-identical to the tiled kernel.
//
// Image: row R < nspan (= 128 + max(dt) - min(dt)) holds source row m0 + min(dt) + R, clamped
// into [0, T) under KF_CLAMP and zero outside it under KF_ZERO; then one slot per part with an
// edge row (loaded when that part's edge_t falls in the tile), then one all-zero slot (tile
// rows past M, and KF_ZERO rows out of range). 128 bytes per row in the halo kernel's layout
// (halo_off: conflict-free for 16 consecutive rows from any first row). Each lane keeps, per
// 16-row group and part, the image row it reads: edge rows, zero rows and the scratch row of
// the row-subsampled stack are only different entries of that table.
//
// One barrier per chunk: both parts' MFMAs (4 sub-steps) run behind one wait. Measured on this
// shape (profiles/r07_splice_phase_parts.txt), a step of the tiled kernel is not latency-bound:
// its wait and barrier, its fragment reads and MFMAs, and the issue of its LDS-DMA pieces run one
// after the other in each wave and add up to the step whether or not the loads were issued
// chunks ahead. So the gain is in what a chunk no longer does: one of two barriers and waits,
// and 16 of its 72 LDS-DMA pieces.
//
// LDS: nimg (4, else 3) images in a ring, so nimg - 2 images are in flight beyond the one
// being read, and B (weights, from L2) in two stages of two 64-row slabs (a chunk's part-0 and
// part-1 slab), the next chunk's stage in flight across the barrier. Every wave issues its share
// of both streams (an LDS-DMA piece costs its issuing wave 100-200 cycles, so the pieces are
// spread evenly over eight waves); vmcnt is per wave and loads retire in order, so the wait is
// counted. Workgroup barriers and vmcnt waits only.
// ---------------------------------------------------------------------------
constexpr int SPL_MAX_PIECES = 20;  // image rows <= 128 + 16 + 2 + 1
struct SpliceArgs {
    const h16 *x;          // A's source rows
    unsigned ldb;          // source row pitch in bytes
    int T, tclamp, pw;
    int dt[2], et[2], er[2];
    int eslot[2];          // image row of part p's edge row
    int lo;                // min(dt)
    int nspan;             // image rows that map to source rows m0 + lo + R
    int zrow;              // the all-zero image row
    int npieces;           // 1 KiB LDS-DMA pieces per image
    int img_bytes, nimg, nch;
    unsigned long long *trace;  // kf_gemm_trace (gemm_kernel's slots), null = off
    int trace_blk;
};

// s_waitcnt vmcnt(n) for a wave-uniform run-time n <= 5 (a wave's pieces of one image); any other
// n waits for everything
__device__ __forceinline__ void wait_vmcnt_img(int n) {
    switch (n) {
        case 1: wait_vmcnt<1>(); break;
        case 2: wait_vmcnt<2>(); break;
        case 3: wait_vmcnt<3>(); break;
        case 4: wait_vmcnt<4>(); break;
        case 5: wait_vmcnt<5>(); break;
        default: wait_vmcnt<0>(); break;
    }
}

template <int BN, bool BKC, int BMODE, int STB, int WM>
__global__ __launch_bounds__(128 * WM, 1) void splice_once_kernel(int M, int N, int K, OpD B, KfEpilogue E,
                                                                  SpliceArgs S, int n_mtiles, int n_ntiles) {
    constexpr int BM = 128, WN = 2, NW = WM * WN;
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 16, TN = WTN / 16;
    static_assert(TN * 16 == WTN && TM * 16 == WTM, "wave tile multiple of 16");
    constexpr int B_STAGE = BN * BK * 2;
    using SB = Stager<BKC, BN, BMODE, NW>;
    static_assert(STB == 4, "two B stages of two slabs (a chunk's part-0 and part-1 slab) each");
    constexpr int MAXQ = (SPL_MAX_PIECES + NW - 1) / NW;  // image pieces per wave
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    char *const bring = dsm + S.nimg * S.img_bytes;  // STB B stages after the images

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int bid = blockIdx.x;
    const bool trb = S.trace != nullptr && tid == 0, trp = trb && bid == S.trace_blk;
    if (trb) {
        S.trace[64 + 3 * bid] = wall_clock64();
        S.trace[64 + 3 * bid + 2] = (unsigned long long)__builtin_amdgcn_s_getreg((4) | (31 << 11)) |
                                    ((unsigned long long)__builtin_amdgcn_s_getreg((20) | (31 << 11)) << 32);
    }
#define SPL_TP(slot) \
    if (trp) S.trace[slot] = wall_clock64();
    SPL_TP(0);
    if (trb && bid == 0) {
        S.trace[60] = (unsigned long long)M | ((unsigned long long)N << 20) | ((unsigned long long)K << 40);
        S.trace[61] = (unsigned long long)BM | ((unsigned long long)BN << 16) | ((unsigned long long)gridDim.x << 32);
        S.trace[62] = 1;
    }

    // XCD-aware tile order (as gemm_kernel): the N tiles of one M tile share an XCD
    const int ntiles = n_mtiles * n_ntiles;
    int tile = blockIdx.x;
    if (ntiles >= 8) {
        const int q = ntiles / 8, rmd = ntiles % 8, xcd = tile % 8, loc = tile / 8;
        tile = (xcd < rmd ? xcd * (q + 1) : rmd * (q + 1) + (xcd - rmd) * q) + loc;
    }
    const int mt = tile / n_ntiles, nt = tile - mt * n_ntiles;
    const int m0 = mt * BM, n0 = nt * BN;

    SB sb;
    sb.init(B, n0, wave, lane);
    const Rsrc rx = make_rsrc(S.x), rb = make_rsrc(B.base);

    // This wave's image pieces q = wave, wave + NW, ..: lane l fills 16-byte position l of a
    // piece, chunk kc of row 8q + r with halo_off(R, kc) = 1024 q + 16 l (conv_halo.hip:
    // halo_issue). Per piece the source byte offset of that row and chunk at column chunk 0
    // (BAD: reads as zero), kept in registers so that a piece costs one add per chunk
    unsigned aoff[MAXQ];
    {
        const int slot = lane & 15, kc = 2 * (lane >> 4) + (slot & 1), r = ((slot - kc) & 15) >> 1;
        const int src0 = m0 + S.lo;  // source row of image row 0
        static_for<MAXQ>([&](auto Q) {
            const int R = 8 * (wave + decltype(Q)::value * NW) + r;
            unsigned ro = BAD;
            if (R < S.nspan) {
                int st = src0 + R;
                if (S.tclamp) st = min(max(st, 0), S.T - 1);
                if ((unsigned)st < (unsigned)S.T) ro = (unsigned)st * S.ldb;
            } else if (R != S.zrow) {
                // the edge rows this tile reads (a part's slot stays zero in the other tiles)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    if (R == S.eslot[p] && S.et[p] >= m0 && S.et[p] < min(m0 + BM, M)) ro = (unsigned)S.er[p] * S.ldb;
            }
            aoff[decltype(Q)::value] = ro == BAD ? BAD : ro + (unsigned)(kc * 16);
        });
    }
    // chunk c's image into ring slot img; na: this wave's pieces of an image
    int na = 0;
#pragma unroll
    for (int j = 0; j < MAXQ; ++j) na += wave + j * NW < S.npieces;
    auto img_issue = [&](int c, int img) {
        char *dst = dsm + img * S.img_bytes;
        const unsigned cb = (unsigned)(c * BK * 2);
        static_for<MAXQ>([&](auto Q) {
            const int q = wave + decltype(Q)::value * NW;
            const unsigned o = aoff[decltype(Q)::value];
            if (q < S.npieces) lds_dma<16>(rx, dst + q * 1024, o == BAD ? BAD : o + cb);
        });
    };

    // per lane: the image row of each 16-row group's row, per part
    int ri[2][TM];
    static_for<TM>([&](auto I) {
        const int r = wm * WTM + I * 16 + (lane & 15), m = m0 + r;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int R = S.zrow;
            if (m < M) {
                const int st = m + S.dt[p];
                if (m == S.et[p]) R = S.eslot[p];
                else if (S.tclamp || (unsigned)st < (unsigned)S.T) R = r + S.dt[p] - S.lo;
            }
            ri[p][I] = R;
        }
    });

    float4v acc[TM][TN];
    static_for<TM>([&](auto I) {
        static_for<TN>([&](auto J) { acc[I][J] = float4v{0.f, 0.f, 0.f, 0.f}; });
    });
    const EpiPre epre = epi_params<BN, 64 * NW>(E, N, n0, tid);

    const int nch = S.nch;
    // One barrier per chunk. Chunk c reads A columns part * pw + 64 c .. for part 0, then part 1,
    // against the two B slabs of that chunk (a B stage holds both). After the barrier every wave
    // issues its pieces of the B stage of chunk c + 1 and then of the image nimg - 1 chunks ahead.
    // Loads retire in order, so the stage of chunk c (issued in chunk c - 1, before that chunk's
    // image pieces) and everything older, this chunk's image included, have landed once at most
    // those image pieces are in flight.
    for (int c = 0; c < S.nimg - 1 && c < nch; ++c) img_issue(c, c);
    if (nch > 0) {
        sb.issue(B, rb, 0, K, bring, wave, lane);
        sb.issue(B, rb, S.pw, K, bring + B_STAGE, wave, lane);
    }
    SPL_TP(1);
    int ia = 0, ib = 0;  // ring slots of this chunk's image and B stage
    int after = 0;       // this wave's loads issued after the B stage of the chunk about to start
    for (int c = 0; c < nch; ++c) {
        wait_vmcnt_img(after);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (c < 40) SPL_TP(2 + c);
        // every wave is past chunk c - 1's reads: its B stage and its image are free
        after = 0;
        if (c + 1 < nch) {
            char *dst = bring + (ib ^ 1) * (2 * B_STAGE);
            sb.issue(B, rb, (c + 1) * BK, K, dst, wave, lane);
            sb.issue(B, rb, S.pw + (c + 1) * BK, K, dst + B_STAGE, wave, lane);
            if (c + S.nimg - 1 < nch) {
                img_issue(c + S.nimg - 1, ia ? ia - 1 : S.nimg - 1);
                after = na;
            }
        }
        const char *ta = dsm + ia * S.img_bytes;
        static_for<2>([&](auto P) {
            constexpr int p = decltype(P)::value;
            const char *tb = bring + ib * (2 * B_STAGE) + p * B_STAGE;
            static_for<BK / 32>([&](auto SS) {
                constexpr int s = decltype(SS)::value;
                half8 fa[TM], fb[TN];
                static_for<TM>([&](auto I) {
                    fa[I] = *reinterpret_cast<const half8 *>(ta + halo_off(ri[p][I], s * 4 + (lane >> 4)));
                });
                static_for<TN>([&](auto J) { fb[J] = load_frag<BKC, BN>(tb, wn * WTN + J * 16, s, lane); });
                static_for<TM>([&](auto I) {
                    static_for<TN>([&](auto J) {
                        acc[I][J] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[I], fb[J], acc[I][J], 0, 0, 0);
                    });
                });
            });
        });
        __builtin_amdgcn_sched_barrier(0);
        ib ^= 1;
        ia = ia + 1 == S.nimg ? 0 : ia + 1;
    }
    SPL_TP(42);
    fused_epilogue<BM, BN, WM, WN>(acc, dsm, E, M, N, m0, n0, tid, lane, wave, &epre);
    SPL_TP(43);
    if (trb) S.trace[64 + 3 * bid + 1] = wall_clock64();
#undef SPL_TP
}

// ---------------------------------------------------------------------------
// plan and dispatch
// ---------------------------------------------------------------------------
// Test hook (kf_ops.h): 1 (default) = products of the class below run on splice_once_kernel where
// the grid is at most one workgroup per CU, 0 = on the tiled gemm_kernel as before, 2 = on
// splice_once_kernel at every row count (measurements: DESIGN.md §10)
static int g_splice_once = 1;
extern "C" void kf_gemm_debug_splice_once(int on) { g_splice_once = on < 0 ? 0 : on > 2 ? 1 : on; }

constexpr int SPL_STB = 4;  // B slabs in LDS: two stages of a chunk's two
constexpr int SPL_WM = 4;   // eight waves of 32x80 (four of 64x80 measured 50 / 62 us against 46 / 49 us per launch)
struct SplicePlan {
    SpliceArgs S;
    size_t lds;
    bool bkc;
    int span, nedge, rows;
};

// diagnostics: the plan of the calling thread's last dispatch (kf_splice_once_debug_last)
constexpr int KF_SPL_DBG_N = 16;
static thread_local int g_spl_dbg[KF_SPL_DBG_N];

// The plan for (M, N, K, a, b, E), or false when the kernel does not apply (the caller then
// runs the tiled kernel: never an error). Pure: no HIP call, nothing written but P.
static bool splice_once_plan(int M, int N, int K, const OpD &a, const OpD &b, bool bkc, bool f8,
                             const KfEpilogue &E, SplicePlan &P) {
    memset(&P, 0, sizeof P);
    if (f8 || a.mk || b.mk || E.drop || E.out8 || E.row_group) return false;
    if (N != 160 && N != 320) return false;
    // a two-part time splice of wide parts: gemm_kernel's kil condition
    if (op_mode(a) != OP_P2 || a.nparts != 2 || a.pw % BK || a.pw < 8 * BK || K != 2 * a.pw || a.ncols != K) return false;
    if (a.dh[0] || a.dh[1] || a.hsrc < 1 || a.T < 1 || a.tmul != 1 || a.t0) return false;
    if (std::abs(a.dt[0]) > 8 || std::abs(a.dt[1]) > 8) return false;
    // B: plain reduction-major weights, or shifted k-contiguous weight rows (op_wrows)
    if (bkc ? op_mode(b) != OP_P2 : op_mode(b) != OP_SIMPLE) return false;
    if (b.tmul != 1 || b.t0) return false;
    SpliceArgs &S = P.S;
    S.x = a.base;
    S.ldb = a.ldb;
    S.T = a.T;
    S.tclamp = a.tclamp;
    S.pw = a.pw;
    S.lo = std::min(a.dt[0], a.dt[1]);
    P.span = std::max(a.dt[0], a.dt[1]) - S.lo;
    S.nspan = 128 + P.span;
    for (int p = 0; p < 2; ++p) {
        S.dt[p] = a.dt[p];
        S.et[p] = a.et[p];
        S.er[p] = a.er[p];
        S.eslot[p] = S.nspan + P.nedge;
        if (a.et[p] >= 0) ++P.nedge;
    }
    S.zrow = S.nspan + P.nedge;
    P.rows = S.zrow + 1;
    S.npieces = (P.rows + 7) / 8;
    if (S.npieces > SPL_MAX_PIECES) return false;
    S.img_bytes = S.npieces * 1024;
    S.nch = a.pw / BK;
    P.bkc = bkc;
    const size_t epi = 16 * 160 + 32 * EpiMap<80>::LDT * 4 * 2 * SPL_WM;  // fused_epilogue<128, 160, WM, 2>
    for (S.nimg = 4; S.nimg >= 3; --S.nimg) {
        P.lds = std::max((size_t)S.nimg * S.img_bytes + (size_t)SPL_STB * 160 * BK * 2, epi);
        if (P.lds <= 160 * 1024) return true;
    }
    return false;
}

static void splice_dbg_fill(int *v, bool applies, int M, int N, const SplicePlan &P) {
    memset(v, 0, sizeof(int) * KF_SPL_DBG_N);
    v[0] = 1;
    v[1] = applies;
    if (!applies) return;
    const int f[] = {128, 160, P.span, P.nedge, 1, P.rows, P.S.npieces, P.S.nimg, SPL_STB, (int)P.lds,
                     (M + 127) / 128, (N + 159) / 160, P.bkc};
    std::copy(f, f + sizeof f / sizeof f[0], v + 2);
}
extern "C" int kf_splice_once_debug_last(int *out, int n) {
    const int m = std::min(std::max(n, 0), KF_SPL_DBG_N);
    for (int i = 0; out && i < m; ++i) out[i] = g_spl_dbg[i];
    return out ? m : 0;
}
extern "C" int kf_splice_once_debug_plan(int M, int N, int K, const KfOperand *A, const KfOperand *B,
                                         const KfEpilogue *epi, int *out, int n) {
    OpD a, b;
    if (!A || !B || !epi || !to_dev(*A, a, "A") || !to_dev(*B, b, "B")) return -1;
    SplicePlan P;
    const bool ok = A->kcontig && (A->fmt == KF_FMT_MXFP8) == (B->fmt == KF_FMT_MXFP8) &&
                    splice_once_plan(M, N, K, a, b, B->kcontig != 0, A->fmt == KF_FMT_MXFP8, *epi, P);
    int v[KF_SPL_DBG_N];
    splice_dbg_fill(v, ok, M, N, P);
    const int m = std::min(std::max(n, 0), KF_SPL_DBG_N);
    for (int i = 0; out && i < m; ++i) out[i] = v[i];
    return out ? m : 0;
}

template <bool BKC, int BMODE>
static int launch_splice(int M, int N, int K, const OpD &a, const OpD &b, const KfEpilogue &E, const SplicePlan &P) {
    kf_take_pending(__func__);
    constexpr int BM = 128, BN = 160;
    const int mt = (M + BM - 1) / BM, nt = (N + BN - 1) / BN;
    SpliceArgs S = P.S;
    S.trace = kf_gemm_trace_take(&S.trace_blk);
    KfProfRec rec{};
    rec.cls = KF_PROF_FUSED;
    rec.flops = 2.0 * M * N * (double)K;
    rec.m = M;
    rec.n = N;
    rec.k = K;
    rec.tile = BM * 10000 + BN;
    rec.bytes = kf_gemm_alg_bytes(a, b, E, M, N);
    kf_launch(splice_once_kernel<BN, BKC, BMODE, SPL_STB, SPL_WM>, dim3(mt * nt), dim3(128 * SPL_WM), P.lds, &rec, M, N, K, b, E, S, mt,
              nt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kf_report_error("splice-once launch (M=%d N=%d K=%d): %s", M, N, K, hipGetErrorString(e));
        return -1;
    }
    // an edge row whose rows span two row tiles: kf_rows_sum, as gemm_kernel's launch
    if (E.edge_out && E.edge_r0 < E.edge_r1 &&
        (E.edge_r0 / BM != (E.edge_r1 - 1) / BM || E.edge_r1 > M || E.edge_r0 < 0))
        return kf_rows_sum_mask(E.edge_out, E.edge_src ? E.out2 : E.out, E.edge_src ? E.ldo2 : E.ldo, E.edge_r0,
                                E.edge_r1, N, nullptr) < 0 ? -1 : 1;
    return 1;
}

// 1 launched, 0 not applicable (the caller runs the tiled kernel), -1 error
int splice_once_try(int M, int N, int K, const OpD &a, const OpD &b, bool bkc, const KfEpilogue &E) {
    SplicePlan P;
    bool ok = splice_once_plan(M, N, K, a, b, bkc, false, E, P);
    // The row counts that run 128x160 tiles (fused_impl's tile 8: few 384-row blocks), while the
    // grid is one round of one workgroup per CU: the images and the B ring take the CU's LDS, and
    // past 256 workgroups the tiled kernel's two 128x160 workgroups per CU win (DESIGN.md §10:
    // N = 320 at 32,020 rows 142 / 153 us tiled against 167 / 183 us; 96,000 rows on 384x160
    // tiles 118 / 125 us against 138 / 162 us)
    const long long grid = (long long)((M + 127) / 128) * ((N + 159) / 160);
    ok = ok && g_splice_once &&
         (g_splice_once == 2 || ((long long)((M + 383) / 384) * ((N + 159) / 160) < 192 && grid <= 256));
    splice_dbg_fill(g_spl_dbg, ok, M, N, P);
    if (!ok) return 0;
    return bkc ? launch_splice<true, OP_P2>(M, N, K, a, b, E, P) : launch_splice<false, OP_SIMPLE>(M, N, K, a, b, E, P);
}
