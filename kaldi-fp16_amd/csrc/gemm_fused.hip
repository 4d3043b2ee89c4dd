// gemm_fused.hip — kf_gemm_fused / kf_gemm_fused_edge (kf_ops.h): validation, the choice of
// kernel (MXFP8, masked A, conv halo, single-staged splice, tile) and the gemm_kernel instantiations with a
// k-contiguous B. The reduction-major-B ones are gemm_fused_mn.hip's.
#include "gemm_fused.h"

// K-step interleave of two-part spliced A operands (WgradArgs::kil): 1 = on (default),
// 0 = part order. Test hook: kf_gemm_debug_kil (kf_ops.h) compares the two orders.
static int g_kil = 1;
extern "C" void kf_gemm_debug_kil(int on) { g_kil = on != 0; }

static int fused_impl(int M, int N, int K, const KfOperand *A, const KfOperand *B, const KfEpilogue *epi,
                      const WgradArgs *edge);
extern "C" int kf_gemm_fused(int M, int N, int K, const KfOperand *A, const KfOperand *B,
                             const KfEpilogue *epi) {
    return fused_impl(M, N, K, A, B, epi, nullptr);
}
extern "C" int kf_gemm_fused_edge(int M, int N, int K, const KfOperand *A, const KfOperand *B,
                                  const KfEpilogue *epi, void *edge_out, const void *x0, const void *x1,
                                  const void *W, int cols) {
    if (!edge_out || !x0 || !x1 || !W || cols <= 0 || cols % 8 || ((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)W) & 15 ||
        A->fmt != KF_FMT_MXFP8 || M <= 0) {
        kf_report_error("kf_gemm_fused_edge: an MXFP8 product with M > 0, an edge row and 16-byte aligned fp16 "
                        "operands, cols %% 8 == 0 (cols=%d)", cols);
        return -1;
    }
    WgradArgs g{};
    g.eo = (h16 *)edge_out;
    g.ex0 = (const h16 *)x0;
    g.ex1 = (const h16 *)x1;
    g.ew = (const h16 *)W;
    g.ecols = cols;
    return fused_impl(M, N, K, A, B, epi, &g);
}
static int fused_impl(int M, int N, int K, const KfOperand *A, const KfOperand *B, const KfEpilogue *epi,
                      const WgradArgs *edge) {
    if (M <= 0 || N <= 0) return 0;
    OpD a, b;
    if (!to_dev(*A, a, "A") || !to_dev(*B, b, "B")) return -1;
    if (N % 8 != 0) {
        kf_report_error("kf_gemm_fused: N=%d must be a multiple of 8", N);
        return -1;
    }
    if (!A->kcontig) {
        kf_report_error("kf_gemm_fused: A must be k-contiguous");
        return -1;
    }
    if (!B->kcontig && !mn_gen_ok(b, "B")) return -1;
    const KfEpilogue &E = *epi;
    if ((E.out && E.ldo % 8) || (E.out2 && E.ldo2 % 8) || (E.resid && E.ldr % 8) ||
        (E.mask_out && E.ldo % 8)) {
        kf_report_error("kf_gemm_fused: leading dimensions must be multiples of 8");
        return -1;
    }
    if (E.out8 && E.out8_src && !E.out2) {
        kf_report_error("kf_gemm_fused: out8_src = 1 needs out2");
        return -1;
    }
    if (E.row_group < 0 || (E.row_group > 0 && (E.row_stride < E.row_group || E.edge_out || edge))) {
        kf_report_error("kf_gemm_fused: row_group %d / row_stride %d (row_stride >= row_group > 0, no edge row)",
                        E.row_group, E.row_stride);
        return -1;
    }
    if (E.out8 && (N % 32 || E.ldo8 % 32 || !E.scale8)) {
        kf_report_error("kf_gemm_fused: out8 needs N and ldo8 multiples of 32 and scale8");
        return -1;
    }
    WgradArgs G{nullptr, nullptr, 0, 0, g_kil};
    if (edge) {
        G.eo = edge->eo;
        G.ex0 = edge->ex0;
        G.ex1 = edge->ex1;
        G.ew = edge->ew;
        G.ecols = edge->ecols;
    }
    const int am = op_mode(a), bm = op_mode(b);
    const bool f8 = A->fmt == KF_FMT_MXFP8;
    if (f8 != (B->fmt == KF_FMT_MXFP8)) {
        kf_report_error("kf_gemm_fused: both operands must be MXFP8, or neither");
        return -1;
    }
    if (E.row_group && (f8 || a.mk || b.mk)) {
        kf_report_error("kf_gemm_fused: grouped output rows (row_group) need an fp16 conv input gradient");
        return -1;
    }
    if (E.drop) {
        // the forward scales the BatchNorm output, the input gradient out2's value: exactly one
        if (!E.row_seg || (E.scale != nullptr) == (E.out2 != nullptr)) {
            kf_report_error("kf_gemm_fused: drop needs row_seg and exactly one of scale (forward) and out2 (input "
                            "gradient)");
            return -1;
        }
        if (E.row_group || E.out8 || E.beta != 0.f || f8 || a.mk || b.mk || edge || am == OP_GEN || bm == OP_GEN) {
            kf_report_error("kf_gemm_fused: drop does not go with row_group, out8, beta, MXFP8, masked or conv operands");
            return -1;
        }
        if (E.ld_drop < N || E.ld_drop % 8 || ((uintptr_t)E.drop & 15) || ((uintptr_t)E.row_seg & 3)) {
            kf_report_error("kf_gemm_fused: drop needs ld_drop >= N, ld_drop %% 8 == 0 and a 16-byte aligned table "
                            "(ld_drop=%lld N=%d)", E.ld_drop, N);
            return -1;
        }
    }
    if (f8) {
        if (K % 128 || am == OP_GEN || a.edges || bm != OP_SIMPLE) {
            kf_report_error("kf_gemm_fused: MXFP8 needs K %% 128 == 0, a plain or time-spliced A and a "
                            "plain B (K=%d)", K);
            return -1;
        }
        const int K2 = K / 2;  // the kernel counts the reduction in 2-byte units
        if (N % 160 == 0 && N <= 320 && !E.out8) {  // TDNN-F linear (N = bottleneck): no idle columns
            if (am == OP_SIMPLE)
                return launch<384, 160, 4, 2, true, true, false, 2, OP_SIMPLE, OP_SIMPLE, 1>(M, N, K2, a, b, E, G, 1);
            return launch<384, 160, 4, 2, true, true, false, 2, OP_P2, OP_SIMPLE, 1>(M, N, K2, a, b, E, G, 1);
        }
        if (N >= 256) {
            if (am == OP_SIMPLE)
                return launch<256, 256, 2, 4, true, true, false, 2, OP_SIMPLE, OP_SIMPLE, 1>(M, N, K2, a, b, E, G, 1);
            return launch<256, 256, 2, 4, true, true, false, 2, OP_P2, OP_SIMPLE, 1>(M, N, K2, a, b, E, G, 1);
        }
        if (am == OP_SIMPLE)
            return launch<128, 128, 2, 2, true, true, false, 2, OP_SIMPLE, OP_SIMPLE, 1>(M, N, K2, a, b, E, G, 1);
        return launch<128, 128, 2, 2, true, true, false, 2, OP_P2, OP_SIMPLE, 1>(M, N, K2, a, b, E, G, 1);
    }
    if (a.mk || b.mk) {
        // masked A (the TDNN-F affine input gradient on the implicit dz, N = bottleneck):
        // 384x160 tiles for N = 160 / 320, 256x64 for N <= 64, else 128x128
        if (!b.mk && B->kcontig && !E.out8 && ((am == OP_P2 && bm == OP_P2) || (am == OP_SIMPLE && bm == OP_SIMPLE))) {
            const int mt = N % 160 == 0 && N <= 320 ? 5 : N <= 64 ? 2 : 0;
#define KF_MASKED(AM_, BM_)                                                                                    \
    do {                                                                                                       \
        if (mt == 5) return launch<384, 160, 4, 2, true, true, false, 2, AM_ | OP_MASKED, BM_>(M, N, K, a, b, E, G, 1); \
        if (mt == 2) return launch<256, 64, 4, 1, true, true, false, 2, AM_ | OP_MASKED, BM_>(M, N, K, a, b, E, G, 1);  \
        return launch<128, 128, 2, 2, true, true, false, 2, AM_ | OP_MASKED, BM_>(M, N, K, a, b, E, G, 1);               \
    } while (0)
            if (am == OP_P2) KF_MASKED(OP_P2, OP_P2);
            KF_MASKED(OP_SIMPLE, OP_SIMPLE);
#undef KF_MASKED
        }
        kf_report_error("kf_gemm_fused: a masked operand must be A (plain or two-part time splice, with a "
                        "k-contiguous B of the same kind, no MXFP8 copy) (M=%d N=%d K=%d)", M, N, K);
        return -1;
    }
    if (!E.drop) {  // the halo kernel shares fused_epilogue, MXFP8 copy included (BN >= 64)
        const int hr = conv_halo_try(M, N, K, a, b, bm, B->kcontig != 0, E);
        if (hr != 0) return hr < 0 ? -1 : 0;
    }
    if (a.tmul > 1 || a.t0 || b.tmul > 1 || b.t0 || E.row_group) {
        kf_report_error("kf_gemm_fused: time-strided rows (tmul / t0) and grouped output rows (row_group) need a "
                        "conv on the halo kernel (M=%d N=%d K=%d)", M, N, K);
        return -1;
    }
    // long-K N = 160 / 320 products on a two-part spliced A at the 128x160 tiles' row counts: the
    // source rows staged once per 64-column chunk (splice_once.hip; it declines everything else)
    if (!f8) {
        const int sr = splice_once_try(M, N, K, a, b, B->kcontig != 0, E);
        if (sr != 0) return sr < 0 ? -1 : 0;
    }
    // Tiles: 384x160 8-wave for N = 160 / 320; 256x64 for N <= 64; for
    // N >= 256 192x128 (or 128x192, below) 8-wave tiles (80 KB of LDS: two workgroups share a CU and one's
    // epilogue overlaps the other's MFMA loop; the wide K = 320 products write 2-3
    // full-width fp16 tensors; their 32-column wave tiles hold the MXFP8 copy's blocks);
    // 128x128 otherwise.
    int tile = 0;
    if (N % 160 == 0 && N <= 320 && !E.out8) tile = 5;
    else if (N <= 64) tile = 2;
    else if (N >= 256) tile = 6;  // 192x128: 32-column wave tiles, so out8 blocks fit
    // short-K wide products with N % 192 == 0: 128x192 tiles (same 80 KB, two per CU; 12 -> 8
    // column tiles per row block): TDNN-F linear input gradient 281 -> 257 us, affine forward
    // 215 -> 207 us (rocprof A/B/A/B). Not with an MXFP8 copy: its 48-column wave tiles do
    // not hold whole 32-column blocks (and 32x96 wave tiles overflow the epilogue's LDS).
    if (tile == 6 && K <= 640 && N % 192 == 0 && !E.out8) tile = 7;
    // N = 160 / 320 with few row blocks (the row-subsampled TDNN-F stack: M = T / 3): 128x160
    // 4-wave tiles, two workgroups per CU, so that the launch fills the CUs (384x160 at
    // M = 32,020 is 84 workgroups)
    if (tile == 5 && (long long)((M + 383) / 384) * ((N + 159) / 160) < 192) tile = 8;
    // (64x160 tiles instead measured 25.21 against 25.05 ms, same box: not used)
    if (!B->kcontig) return fused_mn(tile, am, bm, M, N, K, a, b, E, G);
    if (E.drop) {  // am, bm are plain or two-part here (checked above)
        if (am == OP_SIMPLE && bm == OP_SIMPLE) return fused_tile_drop<true, OP_SIMPLE, OP_SIMPLE>(tile, M, N, K, a, b, E, G);
        if (am == OP_P2 && bm == OP_SIMPLE) return fused_tile_drop<true, OP_P2, OP_SIMPLE>(tile, M, N, K, a, b, E, G);
        if (am == OP_P2 && bm == OP_P2) return fused_tile_drop<true, OP_P2, OP_P2>(tile, M, N, K, a, b, E, G);
        kf_report_error("kf_gemm_fused: drop with a plain A needs a plain B (M=%d N=%d K=%d)", M, N, K);
        return -1;
    }
    if (am == OP_SIMPLE && bm == OP_SIMPLE) return fused_tile<true, OP_SIMPLE, OP_SIMPLE>(tile, M, N, K, a, b, E, G);
    if (am == OP_P2 && bm == OP_SIMPLE) return fused_tile<true, OP_P2, OP_SIMPLE>(tile, M, N, K, a, b, E, G);
    if (am == OP_P2 && bm == OP_P2) return fused_tile<true, OP_P2, OP_P2>(tile, M, N, K, a, b, E, G);
    return fused_tile<true, OP_GEN, OP_GEN>(tile, M, N, K, a, b, E, G);
}
