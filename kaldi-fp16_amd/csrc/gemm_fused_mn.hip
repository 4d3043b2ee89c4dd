// gemm_fused_mn.hip — the fused product's gemm_kernel instantiations with a reduction-major B
// ([K][N] weights: the forward products), a unit of their own for build time (gemm_fused.h).
#include "gemm_fused.h"

int fused_mn(int tile, int am, int bm, int M, int N, int K, const OpD &a, const OpD &b, const KfEpilogue &E,
             const WgradArgs &G) {
    if (E.drop) {  // a TDNN-F affine forward without the transposed weight copy
        if (bm == OP_SIMPLE && am == OP_SIMPLE) return fused_tile_drop<false, OP_SIMPLE, OP_SIMPLE>(tile, M, N, K, a, b, E, G);
        if (bm == OP_SIMPLE && am == OP_P2) return fused_tile_drop<false, OP_P2, OP_SIMPLE>(tile, M, N, K, a, b, E, G);
        kf_report_error("kf_gemm_fused: drop needs a plain or two-part time-spliced A and a plain B (M=%d N=%d K=%d)", M, N, K);
        return -1;
    }
    if (bm != OP_SIMPLE) return fused_tile<false, OP_GEN, OP_GEN>(tile, M, N, K, a, b, E, G);
    if (am == OP_SIMPLE) return fused_tile<false, OP_SIMPLE, OP_SIMPLE>(tile, M, N, K, a, b, E, G);
    if (am == OP_P2) return fused_tile<false, OP_P2, OP_SIMPLE>(tile, M, N, K, a, b, E, G);
    return fused_tile<false, OP_GEN, OP_SIMPLE>(tile, M, N, K, a, b, E, G);
}
