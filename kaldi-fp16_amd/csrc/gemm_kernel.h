// gemm_kernel.h — the FP16 / MXFP8 MFMA GEMM kernel for gfx950 (MI355X) and its launch.
//
// One kernel template covers every dense contraction of the CNN-TDNN step:
//   forward   Y = epi(X . W)           A k-contiguous (activations), B = W[K][N]
//   input grad dX = epi(dZ . W^T)      A k-contiguous (dZ),  B = W rows (k-contiguous)
//   weight grad dW = X^T . dZ          A and B both reduction-major (split-K, fp32)
//   ABI ops_gemm C = a.A.B + b.C       A k-contiguous, B = [K][N]
// replacing the reference's cublasGemmEx (cpp/cuda/ops.cu:381-392) plus the
// separate splice / transpose / bias / relu / BN / bypass kernels around it
// (internal/nnet/forward.go:589-790, internal/gpu/backward_ops.go:162-253).
// The template lives here so that several units instantiate it, each its own family:
// gemm_fused.hip (k-contiguous B, MXFP8, masked A), gemm_fused_mn.hip (reduction-major B),
// gemm_wgrad.hip (split-K weight gradients). conv_halo.hip shares the fused epilogue.
//
// Structure (4 or 8 waves, WM x WN; each wave owns a (BM/WM) x (BN/WN) sub-tile):
//   * operands are fetched in 16-byte chunks through the KfOperand addressing rule
//     (kf_ops.h), so TDNN splices and conv im2col are never materialised; the Stager
//     (gemm_common.h) moves them global -> LDS by LDS-DMA (buffer_load ... lds), invalid
//     chunks (padding, edges) reading as zero through the buffer range check;
//   * an ST-stage LDS ring (2 in every tile in use): stages kt .. kt + ST - 2 are in flight
//     while stage kt is consumed, one barrier and one counted vmcnt wait per K-step;
//   * k-contiguous tiles live as [rows][BK] with a 16-byte XOR swizzle and are read with
//     ds_read_b128; reduction-major tiles live as [BK][W] with an 8-byte XOR swizzle and
//     are read with ds_read_b64_tr_b16 (hardware transpose) — both images are bank-conflict
//     free for the v_mfma_f32_16x16x32_f16 fragment maps; MXFP8 operands ride the same
//     byte movers, their E8M0 scales a ScaleStager, into v_mfma_scale_f32_16x16x128_f8f6f4;
//   * fused epilogue: accumulators are staged through LDS as fp32 and every lane then owns
//     8 consecutive columns of one row, so bias/BN/bypass operands are read and fp16
//     results written as 16-byte vectors (coalesced).
// Tiles, BM x BN on WM x WN waves:
//   fused  384x160 (4x2), 128x160 (2x2), 256x64 (4x1), 192x128 and 128x192 (2x4, 80 KB: two
//          workgroups per CU), 128x128 (2x2); MXFP8 384x160, 256x256 (2x4), 128x128
//   wgrad  384x160 (4x2), 320x256 / 256x256 / 192x256 (2x4), 256x128 / 192x128 (4x2),
//          256x64 / 192x64 (4x1)
#pragma once
#include "gemm_host.h"
#include "kf_prof.h"

// ---------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------
struct WgradArgs {
    float *slab;        // [splits][M][N] fp32 partials
    float *bias_slab;   // [splits][N] fp32 column sums of B, or nullptr
    int k_per_split;    // multiple of BK
    // > 0: A has two time-shifted parts of one source and part p's M tile j covers the
    // same source columns as tile pair_ps * p + j (N fits one tile). Each XCD then gets
    // whole (column chunk, split) pairs, so the two parts' reads of the same source rows
    // meet in one L2 instead of two
    int pair_ps;
    int kil;            // fused: 1 = alternate the K-steps of a two-part A (KF_GEMM_KIL, default 1)
    // diagnostics (kf_gemm_trace), null = off: [0..63] phase stamps of block trace_blk
    // (tid 0), then per block {start, end, hw id | xcc id << 32}
    unsigned long long *trace;
    int trace_blk;
    // fused MXFP8 only (kf_gemm_fused_edge): the last M tile's workgroups also write the fp16
    // row eo[j] = sum_c ex0[c] ew[j][c] + ex1[c] ew[N + j][c] for their columns j
    h16 *eo;
    const h16 *ex0, *ex1, *ew;
    int ecols;
};

template <int BM, int BN, int ST, int SCB = 0>
struct SmemSize {
    static constexpr int stage = (BM + BN) * BK * 2 + SCB;
    static constexpr int pipe = ST * stage;
    static constexpr int bytes = pipe;
};

// ---------------------------------------------------------------------------
// MXFP8 scale staging: per K-step of 128 fp8 elements every tile row needs the
// 4 E8M0 bytes of its 4 blocks, one dword. Slot s of [A rows | B rows | unused]
// is lane s%64 of LDS-DMA instruction s/64; each wave issues SPW of them, so
// the vmcnt bookkeeping stays uniform. Instructions never straddle A and B
// (BM % 64 == 0), so each has one buffer resource.
// ---------------------------------------------------------------------------
template <int BM, int BN, int NW, int AM>
struct ScaleStager {
    static constexpr int SLOTS = BM + BN;
    static constexpr int SPW = (SLOTS + 64 * NW - 1) / (64 * NW);
    static constexpr int BYTES = SPW * NW * 64 * 4;
    static_assert(BM % 64 == 0, "A scale rows fill whole instructions");
    unsigned b0[SPW], b1[SPW];  // A: part-0 / part-1 row offsets; B: row offset (b1 unused)
    __device__ __forceinline__ void init(const OpD &A, const OpD &B, int m0, int n0, int wave,
                                         int lane) {
        static_for<SPW>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const int slot = (wave * SPW + i) * 64 + lane;
            b0[i] = b1[i] = BAD;
            if (slot < BM) {
                const int r = m0 + slot;
                if (r < A.nrows) {
                    if constexpr (AM == OP_SIMPLE) {
                        b0[i] = (unsigned)r * A.lds;
                    } else {
                        for (int p = 0; p < 2 && p < A.nparts; ++p) {
                            int st = r + A.dt[p];
                            bool ok = true;
                            if (A.tclamp) st = min(max(st, 0), A.T - 1);
                            else ok = (unsigned)st < (unsigned)A.T;
                            if (ok) (p ? b1[i] : b0[i]) = (unsigned)st * A.lds;
                        }
                    }
                }
            } else if (slot < SLOTS) {
                const int n = n0 + slot - BM;
                if (n < B.nrows) b0[i] = (unsigned)n * B.lds;
            }
        });
    }
    // k0 in 2-byte units (the fp16 stagers' unit): fp8 element 2*k0 starts the step
    __device__ __forceinline__ void issue(const OpD &A, const OpD &B, Rsrc ra,
                                          Rsrc rb, int k0, char *dst, int wave,
                                          int lane) {
        const int k8 = 2 * k0;
        static_for<SPW>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const int ins = wave * SPW + i;  // wave-uniform
            const int slot = ins * 64 + lane;
            unsigned voff = BAD;
            const bool isA = ins * 64 < BM;
            if (isA) {
                if (k8 < 2 * A.ncols) {
                    if constexpr (AM == OP_SIMPLE) {
                        if (b0[i] != BAD) voff = b0[i] + (unsigned)(k8 >> 5);
                    } else {
                        const int p = k8 >= A.pw8 ? 1 : 0;
                        const unsigned b = p ? b1[i] : b0[i];
                        if (b != BAD) voff = b + (unsigned)((k8 - p * A.pw8) >> 5);
                    }
                }
            } else if (slot < SLOTS && k8 < 2 * B.ncols && b0[i] != BAD) {
                voff = b0[i] + (unsigned)(k8 >> 5);
            }
            // a wave-uniform branch, not a select: a selected 128-bit resource goes to scratch
            if (isA) lds_dma<4>(ra, dst + ins * 256, voff);
            else lds_dma<4>(rb, dst + ins * 256, voff);
        });
    }
};

// ---------------------------------------------------------------------------
// fused epilogue of a BM x BN tile held as 16x16 accumulators. Per-column
// parameters go to LDS once per workgroup; then every wave stages its
// accumulators through its own LDS region 32 rows at a time and each lane owns 8
// consecutive columns of a row (16-byte global I/O). `smem` must hold
// 4*BN + 32*EpiMap<BN/WN>::LDT*WM*WN floats; every LDS-DMA into it must have landed.
// ---------------------------------------------------------------------------
// the epilogue's per-column parameters of column n0 + tid, loaded before the K loop so
// their latency hides under it (KF_EPI_EARLY=0: loaded in the epilogue)
struct EpiPre {
    float b, s, sh, s2;
};
template <int BN, int NTH>
__device__ __forceinline__ EpiPre epi_params(const KfEpilogue &E, int N, int n0, int tid) {
    static_assert(BN <= NTH, "one column per thread");
    EpiPre p{0.f, 0.f, 0.f, 1.f};
    const int n = n0 + tid;
    if (tid < BN && n < N) {
        if (E.bias) p.b = (float)((const h16 *)E.bias)[n];
        if (E.scale) {
            p.s = E.scale[n];
            p.sh = E.shift[n];
        }
        if (E.scale2) p.s2 = E.scale2[n];
    }
    return p;
}

// Epilogue item map and fp32 staging layout of a wave's 32-row chunk. Item k of a lane is
// (row r, 8-column group cg); the lane reads columns 8cg .. 8cg+7 of row r as two 16-byte
// LDS reads and owns them for the global I/O (CG consecutive lanes cover a row's 16 * CG
// contiguous bytes). Rows of WTN + 4 dwords, except for WTN = 64 (the conv halo tiles and
// the 256x256 / 128x128 / 256x64 GEMM tiles): rows of 64 dwords with 16-byte unit u of row r
// at u ^ xr(r), which makes both the accumulator stores and the 16-byte reads bank-conflict
// free (scripts/epi_lds_check.py; the padded rows are 2-way conflicted on the reads: with
// 8-column items a row covers only every other 16-byte unit). For WTN = 32 / 48 (the 80 KB
// 192x128 / 128x192 tiles) the conflicts stay: r5 measured a conflict-free form (the MFMAs
// producing C^T, one 16-byte store per accumulator, rows of 48 dwords, 4-lane row runs) at
// +6 % on the TDNN-F input gradient (257 -> 272 us: its 32-byte global row runs for the last
// 16 columns cost more than the LDS cycles saved), and an XOR mixing lane and loop-index
// bits at 18 more VGPRs (the second workgroup per CU lost, +50 %).
template <int WTN>
struct EpiMap {
    static constexpr int CG = WTN / 8;
    static constexpr bool SWZ = WTN == 64;
    static constexpr int LDT = SWZ ? 64 : WTN + 4;
    __device__ __forceinline__ static int row(int k, int lane) { return (lane + 64 * k) / CG; }
    __device__ __forceinline__ static int cg(int k, int lane) { return (lane + 64 * k) % CG; }
    __device__ __forceinline__ static int xr(int r) { return ((r >> 1) & 1) | (((r >> 2) & 1) << 2); }
    // dword offset of column c of row r
    __device__ __forceinline__ static int off(int r, int c) {
        if constexpr (SWZ) return r * LDT + 4 * ((c >> 2) ^ xr(r)) + (c & 3);
        else return r * LDT + c;
    }
};

// RG: the epilogue honours KfEpilogue.row_group (the conv input-gradient halo kernels only:
// the row map's registers cost the 80 KB GEMM tiles their second workgroup per CU)
// DR: the epilogue applies KfEpilogue.drop (the per-sequence dropout factor, kf_ops.h): a
// compile-time variant, so that every launch without drop keeps the code it had. The tile's
// row -> segment map (rsg: row_seg[m0 + tid], loaded before the K loop like the column
// parameters) goes to LDS behind them, `smem` then holding BM more dwords. The 8 factors of an
// item (two 16-byte loads from a table that lives in L2) sit in ONE register slot per item: a
// second slot, filled with the other row operands a chunk ahead, is 8 * ITEMS more registers
// and costs the 80 KB tiles their second workgroup per CU (128x192: 126 -> 172 VGPRs). So chunk
// 0's factors are issued with the first prefetch, before any store, and item k of chunk
// ic + 1 is issued right after item k of chunk ic has used the slot: a chunk ahead of its use,
// behind that item's own stores only, so its wait never queues behind stores that are still
// in flight when it is needed. The variant takes no beta (old C) operand (host-checked): its
// registers pay for the slot. DESIGN.md §21 lists what each tile uses.
template <int BM, int BN, int WM, int WN, bool RG = false, bool DR = false>
__device__ __forceinline__ void fused_epilogue(float4v (&acc)[BM / WM / 16][BN / WN / 16], char *smem,
                                               const KfEpilogue &E, int M, int N, int m0, int n0,
                                               int tid, int lane, int wave, const EpiPre *pre = nullptr,
                                               int rsg = 0) {
    constexpr int NW = WM * WN, NTH = 64 * NW;
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 16, TN = WTN / 16;
    const int wm = wave / WN, wn = wave % WN;
    // grouped output rows (KfEpilogue.row_group): the address row of GEMM row m
    const int rg = RG ? E.row_group : 0;
    auto arow = [&](int m) -> long long {
        if (!RG || rg <= 0) return m;
        const int g = m / rg;
        return (long long)g * E.row_stride + (m - g * rg);
    };
    static_assert(!DR || BM <= NTH, "one row of the segment map per thread");
    wait_vmcnt<0>();
    __syncthreads();
    float *prm = reinterpret_cast<float *>(smem);
    {
        const EpiPre p = pre ? *pre : epi_params<BN, NTH>(E, N, n0, tid);
        if (tid < BN) {
            prm[tid] = p.b;
            prm[BN + tid] = p.s;
            prm[2 * BN + tid] = p.sh;
            prm[3 * BN + tid] = p.s2;
        }
        if constexpr (DR) {
            if (tid < BM) reinterpret_cast<int *>(prm + 4 * BN)[tid] = rsg;
        }
    }
    __syncthreads();
    const EpiCols P{prm, prm + BN, prm + 2 * BN, prm + 3 * BN};
    using EM = EpiMap<WTN>;
    constexpr int LDT = EM::LDT;
    const int *segl = reinterpret_cast<const int *>(prm + 4 * BN);  // DR: segment of tile row
    float *st = prm + 4 * BN + (DR ? BM : 0) + wave * 32 * LDT;
    constexpr int CG = WTN / 8;
    constexpr int ITEMS = 32 * CG / 64;
    static_assert(ITEMS * 64 == 32 * CG, "items per lane");
    static_assert(TM % 2 == 0, "epilogue stages 32 rows");
    // Row operands (residual, old C, input mask) of the 32-row chunks. The residual rows
    // sit in a ring of NSL register slots, the others in two: chunk ic + NSL - 1 (ic + 1)
    // is issued while chunk ic is processed. When the whole wave tile fits (NSL = TM / 2,
    // small ITEMS), every chunk's residual loads are issued before the first chunk's
    // stores, so no chunk's wait queues behind an earlier chunk's stores (vmcnt is in
    // order): one memory round trip per tile for the bypass epilogue, not one per chunk.
    constexpr int NCH = TM / 2;
    constexpr int NSL = (NCH <= 4 && ITEMS * NCH <= 6) ? NCH : 2;
    half8 rres[NSL][ITEMS], cold[2][ITEMS];
    unsigned mb[2][ITEMS];
    Drop8 dr[DR ? ITEMS : 1];
    auto load_drop = [&](auto ICc, auto K) {
        constexpr int icp = decltype(ICc)::value, k = decltype(K)::value;
        const int r = EM::row(k, lane), cg = EM::cg(k, lane);
        const int ml = wm * WTM + icp * 32 + r, n = n0 + wn * WTN + 8 * cg;
        dr[k].lo = dr[k].hi = float4v{1.f, 1.f, 1.f, 1.f};
        if (m0 + ml < M && n < N) {
            const float4v *q = reinterpret_cast<const float4v *>(E.drop + (long long)segl[ml] * E.ld_drop + n);
            dr[k].lo = q[0];
            dr[k].hi = q[1];
        }
    };
    auto prefetch_res = [&](auto ICc) {
        constexpr int icp = decltype(ICc)::value, sl = icp % NSL;
        static_for<ITEMS>([&](auto K) {
            constexpr int k = decltype(K)::value;
            const int r = EM::row(k, lane), cg = EM::cg(k, lane);
            const int m = m0 + wm * WTM + icp * 32 + r, n = n0 + wn * WTN + 8 * cg;
            rres[sl][k] = half8{};
            if (m < M && n < N && E.resid) rres[sl][k] = load_h8((const h16 *)E.resid + arow(m) * E.ldr + n);
        });
    };
    auto prefetch = [&](auto ICc) {
        constexpr int icp = decltype(ICc)::value, sl = icp & 1;
        static_for<ITEMS>([&](auto K) {
            constexpr int k = decltype(K)::value;
            const int r = EM::row(k, lane), cg = EM::cg(k, lane);
            const int m = m0 + wm * WTM + icp * 32 + r, n = n0 + wn * WTN + 8 * cg;
            const bool ok = m < M && n < N;
            cold[sl][k] = half8{};
            mb[sl][k] = 0xFFu;
            if constexpr (!DR) {
                if (ok && E.beta != 0.f) cold[sl][k] = load_h8((const h16 *)E.out + arow(m) * E.ldo + n);
            }
            if (ok && E.mask_in) mb[sl][k] = E.mask_in[(arow(m) * E.ldo2 + n) >> 3];
        });
    };
    static_for<NSL - 1>([&](auto IC) { prefetch_res(IC); });
    prefetch(std::integral_constant<int, 0>{});
    if constexpr (DR) static_for<ITEMS>([&](auto K) { load_drop(std::integral_constant<int, 0>{}, K); });
    static_for<NCH>([&](auto IC) {
        constexpr int ic = decltype(IC)::value, sl = ic & 1, slr = ic % NSL;
        // (DR: after this chunk's accumulators have gone to LDS and freed their registers; still
        // ahead of the chunk's first store)
        if constexpr (!DR) {
            if constexpr (ic + NSL - 1 < NCH) prefetch_res(std::integral_constant<int, ic + NSL - 1>{});
            if constexpr (ic + 1 < NCH) prefetch(std::integral_constant<int, ic + 1>{});
        }
        static_for<2>([&](auto I2) {
            static_for<TN>([&](auto J) {
                const int c = J * 16 + (lane & 15);
                static_for<4>([&](auto EI) {
                    const int r = I2 * 16 + 4 * (lane >> 4) + EI;
                    st[EM::off(r, c)] = acc[2 * ic + I2][J][decltype(EI)::value];
                });
            });
        });
        if constexpr (DR) {
            if constexpr (ic + NSL - 1 < NCH) prefetch_res(std::integral_constant<int, ic + NSL - 1>{});
            if constexpr (ic + 1 < NCH) prefetch(std::integral_constant<int, ic + 1>{});
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        static_for<ITEMS>([&](auto K) {
            constexpr int k = decltype(K)::value;
            const int r = EM::row(k, lane), cg = EM::cg(k, lane);
            const int nl = wn * WTN + 8 * cg;
            const int m = m0 + wm * WTM + ic * 32 + r, n = n0 + nl;
            const bool live = m < M && n < N;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (live) {
                float4v x0 = *reinterpret_cast<const float4v *>(st + EM::off(r, 8 * cg));
                float4v x1 = *reinterpret_cast<const float4v *>(st + EM::off(r, 8 * cg + 4));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = x0[e];
                    v[e + 4] = x1[e];
                }
                if constexpr (DR) epilogue8<true>(E, P, arow(m), n, nl, v, cold[sl][k], rres[slr][k], mb[sl][k], &dr[k]);
                else epilogue8(E, P, arow(m), n, nl, v, cold[sl][k], rres[slr][k], mb[sl][k]);
            }
            if constexpr (DR && ic + 1 < NCH) load_drop(std::integral_constant<int, ic + 1>{}, K);
            if constexpr (CG % 4 == 0 && !DR) {
                // MXFP8 copy: the 4 lanes l..l+3 (l % 4 == 0) hold one 32-column block
                if (E.out8) {
                    float amax = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
                    amax = fmaxf(amax, __shfl_xor(amax, 1));
                    amax = fmaxf(amax, __shfl_xor(amax, 2));
                    const int ex = mx_exponent(amax);
                    const float inv = __uint_as_float((unsigned)(127 - ex) << 23);
                    float q[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) q[e] = v[e] * inv;
                    const uint2 pk = pack_e4m3x8(q);
                    if (live) {
                        const long long ma = arow(m);
                        *reinterpret_cast<uint2 *>((uint8_t *)E.out8 + ma * E.ldo8 + n) = pk;
                        if ((lane & 3) == 0) E.scale8[ma * (E.ldo8 >> 5) + (n >> 5)] = (uint8_t)(ex + 127);
                    }
                }
            }
        });
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    });
    // edge row (KfEpilogue.edge_out): the row tile that holds rows [edge_r0, edge_r1) sums the
    // values it just stored, per column in row order (kf_rows_sum's order and rounding), once
    // every wave's stores are visible to the workgroup. The host falls back to kf_rows_sum when
    // the rows span two tiles (launch<>). Visibility rests on CU mode with the write-through
    // L1 (the workgroup-scope release / acquire below) and on no earlier read of out / out2
    // in this kernel (a beta accumulation reads out, but only rows it then overwrites, and
    // edge_src = 1 sums out2, which nothing reads before); a change to either needs a
    // different source, e.g. the fp32 staging rounded as stored.
    if (E.edge_out && E.edge_r0 >= m0 && E.edge_r1 <= m0 + BM && E.edge_r1 <= M && E.edge_r0 < E.edge_r1) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const h16 *src = (const h16 *)(E.edge_src ? E.out2 : E.out);
        const long long ld = E.edge_src ? E.ldo2 : E.ldo;
        for (int c = tid; c < BN; c += NTH) {
            const int n = n0 + c;
            if (n >= N) continue;
            float s = 0.f;
            for (int r = E.edge_r0; r < E.edge_r1; ++r) s += h2f(src[(long long)r * ld + n]);
            ((h16 *)E.edge_out)[n] = f2h(s);
        }
    }
}

template <int BM, int BN, int WM, int WN, bool AKC, bool BKC, bool WGRAD, int ST, int AM, int BMODE,
          int F8 = 0>
__global__ __launch_bounds__(64 * WM * WN, 1) void gemm_kernel(int M, int N, int K, OpD A, OpD B,
                                                               KfEpilogue E, WgradArgs G,
                                                               int n_mtiles, int n_ntiles) {
    constexpr int NW = WM * WN, NTH = 64 * NW;
    // operand modes; bit 3 (OP_MASKED) = the operand carries a bit mask (KfOperand.mask)
    constexpr int AMD = AM & 7, BMD = BMODE & 7;
    constexpr bool AMK = (AM & OP_MASKED) != 0, BMK = (BMODE & OP_MASKED) != 0, MK = AMK || BMK;
    // bit 4 of the A mode (EPI_DROP): the epilogue applies KfEpilogue.drop to the rows A names
    constexpr bool DR = (AM & EPI_DROP) != 0;
    static_assert(!DR || (!WGRAD && !F8 && !MK), "drop: fp16 fused products without masked operands");
    static_assert(!MK || (ST == 2 && !F8), "masked operands: two-stage ring, fp16");
    using SCS = ScaleStager<F8 ? BM : 64, F8 ? BN : 64, NW, AMD>;  // used by MXFP8 only
    constexpr int SCB = F8 ? SCS::BYTES : 0;
    static_assert(!F8 || (AKC && BKC && !WGRAD && BMD == OP_SIMPLE && AMD != OP_GEN),
                  "MXFP8: k-contiguous plain / spliced A, plain B");
    static_assert(NW == 4 || NW == 8, "4 or 8 waves");
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 16, TN = WTN / 16;
    static_assert(TM * 16 == WTM && TN * 16 == WTN, "wave tile multiple of 16");
    constexpr int A_STAGE = BM * BK * 2, B_STAGE = BN * BK * 2;
    constexpr int STAGE = A_STAGE + B_STAGE + SCB;
    using SA = Stager<AKC, BM, AMD, NW, AMK>;
    using SB = Stager<BKC, BN, BMD, NW, BMK>;
    constexpr int LPT = SA::NC + SB::NC + (F8 ? SCS::SPW : 0);  // LDS-DMA per thread per stage
    static_assert((SA::EVEN && SB::EVEN) || ST == 2, "uneven stagers need the vmcnt(0) ring");
    static_assert(ST >= 2 && ST <= 4, "stages");
    static_assert(WGRAD || 4 * BN * 4 + (DR ? BM * 4 : 0) + (32 * EpiMap<WTN>::LDT * 4) * NW <=
                               SmemSize<BM, BN, ST, SCB>::bytes,
                  "epilogue staging");

    __shared__ __attribute__((aligned(16))) char smem[SmemSize<BM, BN, ST, SCB>::bytes + (MK ? 4096 : 0)];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int bid = blockIdx.x + blockIdx.y * gridDim.x;
    const bool trb = G.trace != nullptr && tid == 0, trp = trb && bid == G.trace_blk;
    if (trb) {
        G.trace[64 + 3 * bid] = wall_clock64();
        G.trace[64 + 3 * bid + 2] = (unsigned long long)__builtin_amdgcn_s_getreg((4) | (31 << 11)) |
                                    ((unsigned long long)__builtin_amdgcn_s_getreg((20) | (31 << 11)) << 32);
    }
#define GEMM_TP(slot) \
    if (trp) G.trace[slot] = wall_clock64();
    GEMM_TP(0);
    if (trb && bid == 0) {
        G.trace[60] = (unsigned long long)M | ((unsigned long long)N << 20) | ((unsigned long long)K << 40);
        G.trace[61] = (unsigned long long)BM | ((unsigned long long)BN << 16) | ((unsigned long long)gridDim.x << 32);
        G.trace[62] = gridDim.y;
    }

    // XCD-aware tile order: consecutive tile ids (the N tiles of one M tile, which
    // share the A rows) land on one XCD, whose L2 then serves the A re-reads.
    const int ntiles = n_mtiles * n_ntiles;
    int tile = blockIdx.x;
    if (ntiles >= 8) {
        const int q = ntiles / 8, rmd = ntiles % 8, xcd = tile % 8, loc = tile / 8;
        tile = (xcd < rmd ? xcd * (q + 1) : rmd * (q + 1) + (xcd - rmd) * q) + loc;
    }
    int split = blockIdx.y;
    if constexpr (WGRAD) {
        if (G.pair_ps > 0) {
            const int total = gridDim.x * gridDim.y, L = blockIdx.x + blockIdx.y * gridDim.x;
            const int q = total / 8, rmd = total % 8, xcd = L % 8, loc = L / 8;
            const int w = (xcd < rmd ? xcd * (q + 1) : rmd * (q + 1) + (xcd - rmd) * q) + loc;
            const int unit = w >> 1, chunk = unit / gridDim.y;
            split = unit - chunk * gridDim.y;
            tile = (w & 1) * G.pair_ps + chunk;  // n_ntiles == 1
        }
    }
    const int mt = tile / n_ntiles, nt = tile - mt * n_ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    int kbeg = 0, kend = K;
    if constexpr (WGRAD) {
        kbeg = split * G.k_per_split;
        kend = min(K, kbeg + G.k_per_split);
    }
    const int nk = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;

    SA sa;
    SB sb;
    SCS ss;
    sa.init(A, m0, wave, lane);
    sb.init(B, n0, wave, lane);
    if constexpr (F8) ss.init(A, B, m0, n0, wave, lane);
    const Rsrc ra = make_rsrc(A.base), rb = make_rsrc(B.base);
    Rsrc rsa = ra, rsb = rb;
    if constexpr (F8) {
        rsa = make_rsrc(A.sc);
        rsb = make_rsrc(B.sc);
    }
    auto issue = [&](int stage, int k0) {
        char *base = smem + stage * STAGE;
        sa.issue(A, ra, k0, kend, base, wave, lane);
        sb.issue(B, rb, k0, kend, base + A_STAGE, wave, lane);
        if constexpr (F8) ss.issue(A, B, rsa, rsb, k0, base + A_STAGE + B_STAGE, wave, lane);
    };

    float4v acc[TM][TN];
    static_for<TM>([&](auto I) {
        static_for<TN>([&](auto J) { acc[I][J] = float4v{0.f, 0.f, 0.f, 0.f}; });
    });

    const bool do_bsum = WGRAD && G.bias_slab != nullptr && mt == 0 && !BKC;
    float bsum = 0.f;

    // ST-stage LDS ring: stages kt .. kt+ST-2 are in flight while kt is consumed;
    // the counted wait retires only stage kt (never vmcnt(0) in steady state)
    // (plain statements: a lambda around `issue` makes the stager's offset arrays
    // address-taken and sends them to scratch)
    EpiPre epre{0.f, 0.f, 0.f, 1.f};
    if constexpr (!WGRAD) epre = epi_params<BN, 64 * NW>(E, N, n0, tid);
    int rsg = 0;  // DR: the segment of tile row tid (KfEpilogue.row_seg), for the epilogue
    if constexpr (DR) {
        if (tid < BM && m0 + tid < M) rsg = E.row_seg[m0 + tid];
    }
    // a two-part k-contiguous A ([x(t + d0) | x(t + d1)], K = 2 x part width): the K-steps
    // alternate between the parts, so each 64-column chunk of the source rows is fetched
    // for both parts while it is still in L2 (in part order the second pass misses)
    int kil = 0;
    if constexpr (!WGRAD && !F8 && AKC && AMD == OP_P2)
        // (wide parts only: a narrow part's second pass is a few K-steps away and still hits)
        kil = (A.nparts == 2 && A.pw % BK == 0 && A.pw >= 8 * BK && K == 2 * A.pw && G.kil) ? A.pw : 0;
    auto kofs = [&](int kt) { return kbeg + (kil ? (kt & 1) * kil + (kt >> 1) * BK : kt * BK); };
    uint4 *const mlut = reinterpret_cast<uint4 *>(smem + ST * STAGE);
    if constexpr (MK) {
        mask_lut_fill(mlut, tid, NTH);
        __syncthreads();
    }
    if (nk > 0) issue(0, kofs(0));
    if (ST >= 3 && nk > 1) issue(1, kofs(1));
    if (ST >= 4 && nk > 2) issue(2, kofs(2));
    GEMM_TP(1);
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + ST - 2 < nk) wait_vmcnt<LPT * (ST - 2)>();
        else wait_vmcnt<0>();
        if constexpr (MK) {
            // ST == 2: the wait above retired this stage's chunks and mask bytes
            char *stg = smem + (kt % ST) * STAGE;
            if constexpr (AMK) sa.apply_mask(stg, mlut, wave, lane);
            if constexpr (BMK) sb.apply_mask(stg + A_STAGE, mlut, wave, lane);
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the masked chunks are in LDS
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (kt < 40) GEMM_TP(2 + kt);
        if (kt + ST - 1 < nk) issue((kt + ST - 1) % ST, kofs(kt + ST - 1));
        const char *ta = smem + (kt % ST) * STAGE;
        const char *tb = ta + A_STAGE;
        if constexpr (F8) {
            // one v_mfma_scale_f32_16x16x128_f8f6f4 per (I, J) per K-step: lane l holds
            // bytes [16g, 16g+16) and [64+16g, 64+16g+16) of its row (g = l>>4) — the
            // chunks the fp16 fragment loads of s = 0, 1 return — and supplies the
            // E8M0 scale of block g of row l&15 (lane maps measured on the MI355X,
            // scripts/probe_mx.py)
            const unsigned *sct = reinterpret_cast<const unsigned *>(tb + B_STAGE);
            const int g8 = 8 * (lane >> 4);
            typedef int v8i __attribute__((ext_vector_type(8)));
            v8i fa[TM], fb[TN];
            int sca[TM], scb[TN];
            static_for<TM>([&](auto I) {
                const int r = wm * WTM + I * 16;
                half8 lo = load_frag<true, BM>(ta, r, 0, lane), hi = load_frag<true, BM>(ta, r, 1, lane);
                fa[I] = __builtin_shufflevector(__builtin_bit_cast(v4i_t, lo), __builtin_bit_cast(v4i_t, hi),
                                                0, 1, 2, 3, 4, 5, 6, 7);
                sca[I] = (int)((sct[r + (lane & 15)] >> g8) & 0xFF);
            });
            static_for<TN>([&](auto J) {
                const int c = wn * WTN + J * 16;
                half8 lo = load_frag<true, BN>(tb, c, 0, lane), hi = load_frag<true, BN>(tb, c, 1, lane);
                fb[J] = __builtin_shufflevector(__builtin_bit_cast(v4i_t, lo), __builtin_bit_cast(v4i_t, hi),
                                                0, 1, 2, 3, 4, 5, 6, 7);
                scb[J] = (int)((sct[BM + c + (lane & 15)] >> g8) & 0xFF);
            });
            static_for<TM>([&](auto I) {
                static_for<TN>([&](auto J) {
                    acc[I][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                        fa[I], fb[J], acc[I][J], 0, 0, 0, sca[I], 0, scb[J]);
                });
            });
        } else
        static_for<BK / 32>([&](auto S) {
            constexpr int s = decltype(S)::value;
            half8 fa[TM], fb[TN];
            static_for<TM>([&](auto I) { fa[I] = load_frag<AKC, BM>(ta, wm * WTM + I * 16, s, lane); });
            static_for<TN>([&](auto J) { fb[J] = load_frag<BKC, BN>(tb, wn * WTN + J * 16, s, lane); });
            static_for<TM>([&](auto I) {
                static_for<TN>([&](auto J) {
                    acc[I][J] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[I], fb[J], acc[I][J], 0, 0, 0);
                });
            });
        });
        if constexpr (WGRAD && !BKC) {
            if (do_bsum && tid < BN) {
                for (int r = 0; r < BK; ++r) {
                    const char *p = tb + mn_off<BN>(r, tid >> 2) + 2 * (tid & 3);
                    bsum += (float)*reinterpret_cast<const h16 *>(p);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    if constexpr (WGRAD) {
        float *slab = G.slab + (long long)split * M * N;
        static_for<TM>([&](auto I) {
            static_for<TN>([&](auto J) {
                const int n = n0 + wn * WTN + J * 16 + (lane & 15);
                static_for<4>([&](auto EI) {
                    const int m = m0 + wm * WTM + I * 16 + 4 * (lane >> 4) + EI;
                    if (m < M && n < N) slab[(long long)m * N + n] = acc[I][J][decltype(EI)::value];
                });
            });
        });
        if (do_bsum && tid < BN && n0 + tid < N)
            G.bias_slab[(long long)split * N + n0 + tid] = bsum;
    } else {
        GEMM_TP(42);
        fused_epilogue<BM, BN, WM, WN, false, DR>(acc, smem, E, M, N, m0, n0, tid, lane, wave, &epre, rsg);
        if constexpr (F8) {
            if (G.eo && mt == n_mtiles - 1) {
                // the clamped-edge row of the TDNN-F affine input gradient in fp16 (its second
                // part is a sum of rows, which the MXFP8 operand does not hold): one wave per
                // output column, 8-element chunks per lane, fixed-order wave reduction
                for (int j = n0 + wave; j < min(n0 + BN, N); j += NW) {
                    const h16 *w0 = G.ew + (long long)j * G.ecols, *w1 = G.ew + (long long)(N + j) * G.ecols;
                    float a = 0.f;
                    for (int c = 8 * lane; c < G.ecols; c += 8 * 64) {
                        const half8 x = load_h8(G.ex0 + c), y = load_h8(G.ex1 + c), u = load_h8(w0 + c),
                                    v = load_h8(w1 + c);
#pragma unroll
                        for (int e = 0; e < 8; ++e) a = fmaf((float)x[e], (float)u[e], fmaf((float)y[e], (float)v[e], a));
                    }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
                    if (lane == 0) G.eo[j] = f2h(a);
                }
            }
        }
    }
    GEMM_TP(43);
    if (trb) G.trace[64 + 3 * bid + 1] = wall_clock64();
#undef GEMM_TP
}

// launch of one instantiation; splits > 1 for the weight gradient's split-K only. The fused
// product's edge row (KfEpilogue.edge_out) falls back to kf_rows_sum when its rows span two
// row tiles (fused_epilogue).
template <int BM, int BN, int WM, int WN, bool AKC, bool BKC, bool WGRAD, int ST, int AM, int BMODE,
          int F8 = 0>
static int launch(int M, int N, int K, const OpD &A, const OpD &B, const KfEpilogue &E,
                  const WgradArgs &G0, int splits) {
    kf_take_pending(__func__);
    const int mt = (M + BM - 1) / BM, nt = (N + BN - 1) / BN;
    dim3 grid(mt * nt, WGRAD ? splits : 1);
    WgradArgs G = G0;
    G.trace = kf_gemm_trace_take(&G.trace_blk);
    KfProfRec rec{};
    rec.cls = WGRAD ? KF_PROF_WGRAD : KF_PROF_FUSED;
    rec.flops = 2.0 * M * N * (double)K * (F8 ? 2 : 1);  // K counts 2-byte units
    rec.m = M;
    rec.n = N;
    rec.k = K;
    rec.tile = BM * 10000 + BN;
    // A is [M x K] (or its K-major view), B is [K x N]; wgrad writes fp32 dW [M x N]
    rec.bytes = op_src_bytes(A, F8) + op_src_bytes(B, F8) + (WGRAD ? (double)M * N * 4 : epi_bytes(E, M, N));
    kf_launch(gemm_kernel<BM, BN, WM, WN, AKC, BKC, WGRAD, ST, AM, BMODE, F8>, grid, dim3(64 * WM * WN), 0, &rec,
              M, N, K, A, B, E, G, mt, nt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        kf_report_error("gemm launch (M=%d N=%d K=%d): %s", M, N, K, hipGetErrorString(e));
        return -1;
    }
    if (!WGRAD && E.edge_out && E.edge_r0 < E.edge_r1 &&
        (E.edge_r0 / BM != (E.edge_r1 - 1) / BM || E.edge_r1 > M || E.edge_r0 < 0))
        return kf_rows_sum_mask(E.edge_out, E.edge_src ? E.out2 : E.out, E.edge_src ? E.ldo2 : E.ldo, E.edge_r0,
                                E.edge_r1, N, nullptr);
    return 0;
}
