// gemm_fused.h — the fused product's tile dispatch, shared by its two units: gemm_fused.hip
// (validation, tile choice and the k-contiguous-B, MXFP8 and masked instantiations) and
// gemm_fused_mn.hip (the reduction-major-B instantiations). No instantiation is in both.
#pragma once
#include "gemm_kernel.h"

// fused_impl's tile choice (gemm_fused.hip): 8 128x160, 7 128x192, 6 192x128, 5 384x160,
// 2 256x64, else 128x128
template <bool BKC, int AM, int BMODE>
static int fused_tile(int tile, int M, int N, int K, const OpD &a, const OpD &b, const KfEpilogue &E,
                      const WgradArgs &G) {
    if (tile == 8) return launch<128, 160, 2, 2, true, BKC, false, 2, AM, BMODE>(M, N, K, a, b, E, G, 1);
    if (tile == 7) return launch<128, 192, 2, 4, true, BKC, false, 2, AM, BMODE>(M, N, K, a, b, E, G, 1);
    if (tile == 6) return launch<192, 128, 2, 4, true, BKC, false, 2, AM, BMODE>(M, N, K, a, b, E, G, 1);
    if (tile == 5) return launch<384, 160, 4, 2, true, BKC, false, 2, AM, BMODE>(M, N, K, a, b, E, G, 1);
    if (tile == 2) return launch<256, 64, 4, 1, true, BKC, false, 2, AM, BMODE>(M, N, K, a, b, E, G, 1);
    return launch<128, 128, 2, 2, true, BKC, false, 2, AM, BMODE>(M, N, K, a, b, E, G, 1);
}

// the same with KfEpilogue.drop (EPI_DROP): the tiles a TDNN-F's affine forward and the input
// gradients into a TDNN-F run on (N > 64, not 160 / 320)
template <bool BKC, int AM, int BMODE>
static int fused_tile_drop(int tile, int M, int N, int K, const OpD &a, const OpD &b, const KfEpilogue &E,
                           const WgradArgs &G) {
    if (tile == 7) return launch<128, 192, 2, 4, true, BKC, false, 2, AM | EPI_DROP, BMODE>(M, N, K, a, b, E, G, 1);
    if (tile == 6) return launch<192, 128, 2, 4, true, BKC, false, 2, AM | EPI_DROP, BMODE>(M, N, K, a, b, E, G, 1);
    if (tile == 0) return launch<128, 128, 2, 2, true, BKC, false, 2, AM | EPI_DROP, BMODE>(M, N, K, a, b, E, G, 1);
    kf_report_error("kf_gemm_fused: drop has no kernel for this product's tile (N=%d: N > 64 and not 160 / 320)", N);
    return -1;
}

// B reduction-major ([K][N] weights): am / bm are the operands' op_mode
__attribute__((visibility("hidden"))) int fused_mn(int tile, int am, int bm, int M, int N, int K, const OpD &a,
                                                   const OpD &b, const KfEpilogue &E, const WgradArgs &G);
