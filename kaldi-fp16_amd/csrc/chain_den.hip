// chain_den.hip — the probability-space denominator of the chain objective with the
// leaky HMM (chain_den.cu:496-706), G workgroups per sequence (or sequence pair): the
// alpha' / beta state rows and the frame's exp(x) row live in LDS, arcs are streamed from
// SELL-64 tables (chain_tables.cpp builds them), partial sums and state slices cross
// workgroups through a bounded-spin exchange, posteriors accumulate in LDS as 2^-44 fixed
// point. k_den_fwd (forward alone), k_den_fb (both recursions in one launch), k_den_post
// (posteriors; in product mode the whole objective assembly of backward.go:224-371 and
// the fp16 gradient row) and k_perm_gather, with the device tables of a graph and the
// host launch entries (chain_denom.h).
#include "chain_denom.h"

// Row prefetch held in registers between frames: fp16 rows stay packed (2 per VGPR).
// Loads are unconditional (index clamped); the out-of-range select at issue makes the
// fetch wait for its row, which measured faster than a select at use (5.87 vs 6.13 ms
// for k_den_fb: the consume loads then no longer queue behind the HBM row in vmcnt).
template <typename XT> struct RowPre {
    float v[DEN_MAXPT];
    __device__ __forceinline__ void fetch(const XT *row, int P) {
#pragma unroll
        for (int i = 0; i < DEN_MAXPT; ++i) {
            int p = threadIdx.x + i * DEN_THREADS;
            float x = (float)row[min(p, P - 1)];
            v[i] = p < P ? x : 0.0f;
        }
    }
    __device__ __forceinline__ float get(int i, int) const { return v[i]; }
};
template <> struct RowPre<h16> {
    uint32_t v[DEN_MAXPT / 2];
    __device__ __forceinline__ void fetch(const h16 *row, int P) {
        const unsigned short *u = reinterpret_cast<const unsigned short *>(row);
#pragma unroll
        for (int i = 0; i < DEN_MAXPT / 2; ++i) {
            int p0 = threadIdx.x + (2 * i) * DEN_THREADS, p1 = p0 + DEN_THREADS;
            uint32_t lo = __builtin_nontemporal_load(u + min(p0, P - 1));
            uint32_t hi = __builtin_nontemporal_load(u + min(p1, P - 1));
            v[i] = (p0 < P ? lo : 0u) | ((p1 < P ? hi : 0u) << 16);
        }
    }
    __device__ __forceinline__ float get(int i, int) const {
        unsigned short b = (unsigned short)((i & 1) ? (v[i >> 1] >> 16) : (v[i >> 1] & 0xFFFF));
        return (float)__builtin_bit_cast(h16, b);
    }
};
struct StatePre {  // alpha' row prefetch (S <= DEN_MAXS * DEN_THREADS)
    float v[DEN_MAXS];
    __device__ __forceinline__ void fetch(const float *row, int S) {
#pragma unroll
        for (int i = 0; i < DEN_MAXS; ++i) {
            int s = threadIdx.x + i * DEN_THREADS;
            float x = __builtin_nontemporal_load(row + min(s, S - 1));
            v[i] = s < S ? x : 0.0f;
        }
    }
};

// ---------------------------------------------------------------------------
// Cross-workgroup exchange (G workgroups per sequence). Hand-off recipe of
// cdna_hip_programming.md §6 Guideline 16 (R1, counter form, all-sc1): every
// payload word is stored write-through (sc1) by its wave, every storing wave
// drains vmcnt, the workgroup barriers, one lane adds to the sequence's counter
// (agent scope); consumers poll that counter relaxed (bounded, s_sleep), barrier,
// and read every payload word with sc1 loads. Counters and the per-launch timeout
// word are zeroed by hipMemsetAsync before every launch; a block that gives up also
// adds to a sticky word that only kf_chain_result / the den ABI read and clear, so a
// timed-out launch is reported even when later launches succeed.
// ---------------------------------------------------------------------------
typedef __attribute__((address_space(1))) unsigned int gu32_t;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ void st_sc1(float *p, float v) {
    __hip_atomic_store((gu32_t *)p, __float_as_uint(v), RLX_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float *p) {
    return __uint_as_float(__hip_atomic_load((gu32_t *)p, RLX_AGENT));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t den_rsrc(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, (int)0xFFFFFFFF, 0x00020000);
}
// Exchange word access. LOC: every block of the sequence runs on one XCD, so they share
// one L2 — plain stores (written through the CU's L1 into that L2, acknowledged there)
// and sc1 loads (which bypass the reading CU's L1 and are served by that L2) hand the data
// over without the write-through to memory that agent-scope stores need across XCDs.
// (An sc0 load hits the L1 like a plain one: the partial-sum slots, rewritten every other
// frame, then came back stale whenever the state rows were too small to evict them.)
// `base` is uniform, `i` a word index.
template <bool LOC>
__device__ __forceinline__ void x_st(float *base, int i, float v) {
    if constexpr (LOC)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), den_rsrc(base), i * 4, 0, 0);
    else
        st_sc1(base + i, v);
}
template <bool LOC>
__device__ __forceinline__ float x_ld(const float *base, int i) {
    if constexpr (LOC)
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(den_rsrc(base), i * 4, 0, 16 /* sc1 */));
    else
        return ld_sc1(base + i);
}

// unit / slice-owner of this block; the G blocks of a unit share an XCD when the grid
// allows it (blocks b and b+8 share one, MI355X_MICROARCH.md)
__device__ __forceinline__ void den_map(const DenX &X, int &unit, int &gi) {
    const int nb = X.nseq * X.G, b = blockIdx.x;
    int w = b;
    if (nb % 8 == 0 && (nb / 8) % X.G == 0) w = (b % 8) * (nb / 8) + b / 8;
    unit = w >> X.lgG;
    gi = w & (X.G - 1);
}

// publish: every wave stores its NS partial sums (lane 0, tail slots q * DEN_WAVES +
// wave); every wave drains vmcnt, the workgroup barriers, one lane adds the arrival
// (one store drain per frame)
template <bool LOC, int NS>
__device__ __forceinline__ void den_publish(const DenX &X, float *tail, const float (&wsum)[NS], int unit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) x_st<LOC>(tail, q * DEN_WAVES + wave, wsum[q]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add((gu32_t *)&X.cnt[unit], 1u, RLX_AGENT);
}
// one lane polls `word` until done(value); false on timeout, uniform. *val: the last value
template <class Done>
__device__ __forceinline__ bool den_poll(const DenX &X, const unsigned *word, Done done, int *lds_flag,
                                         unsigned *val = nullptr) {
    if (threadIdx.x == 0) {
        int ok = 1;
        for (unsigned it = 0;; ++it) {
            const unsigned v = __hip_atomic_load((gu32_t *)word, RLX_AGENT);
            if (val) *val = v;
            if (done(v)) break;
            if ((it & 255) == 255 && __hip_atomic_load((gu32_t *)X.tmo, RLX_AGENT)) {
                ok = 0;
                break;
            }
            if (it >= X.spin_limit) {  // ~seconds by default: a partner block is not resident
                __hip_atomic_store((gu32_t *)X.tmo, 1u, RLX_AGENT);
                __hip_atomic_fetch_add((gu32_t *)X.sticky, 1u, RLX_AGENT);
                ok = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        *lds_flag = ok;
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return *lds_flag != 0;
}
// wait for `target` arrivals; false on timeout, uniform
__device__ __forceinline__ bool den_wait(const DenX &X, int unit, unsigned target, int *lds_flag) {
    return den_poll(X, &X.cnt[unit], [&](unsigned v) { return v >= target; }, lds_flag);
}
// XCD census before the first exchange: 1 if all G blocks of the unit run on one XCD
// (the placement den_map asks the dispatcher for, not a guarantee), 0 if not or
// forced, -1 on timeout; uniform. Each block adds 1 to its XCD's 4-bit field.
__device__ __forceinline__ int den_xcd_local(const DenX &X, int unit, int *lds_flag) {
    if (unit >= X.nseq) return 0;  // grid padding: no exchange
    unsigned *word = X.xm + unit;
    if (threadIdx.x == 0) {
        const unsigned xcc = __builtin_amdgcn_s_getreg((20) | (3 << 11)) & 7;  // HW_REG_XCC_ID
        __hip_atomic_fetch_add((gu32_t *)word, 1u << (4 * xcc), RLX_AGENT);
    }
    auto total = [](unsigned v) {
        unsigned n = 0;
        for (int k = 0; k < 8; ++k) n += (v >> (4 * k)) & 15;
        return n;
    };
    unsigned *vl = reinterpret_cast<unsigned *>(lds_flag) + 1;
    if (!den_poll(X, word, [&](unsigned v) { return total(v) >= (unsigned)X.G; }, lds_flag, vl)) return -1;
    const unsigned v = *vl;
    bool one = false;
    for (int k = 0; k < 8; ++k)
        if (((v >> (4 * k)) & 15) == (unsigned)X.G) one = true;
    return one && !X.force_sys ? 1 : 0;
}
// NS values per state: the LDS state row is NS-interleaved (one 4 * NS-byte word per state)
template <int NS> struct DenV {
    float x[NS];
};
template <int NS>
__device__ __forceinline__ DenV<NS> lds_v(const unsigned char *base, unsigned off) {
    DenV<NS> r;
    if constexpr (NS == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(base + off);
        r.x[0] = t.x;
        r.x[1] = t.y;
    } else {
        r.x[0] = *reinterpret_cast<const float *>(base + off);
    }
    return r;
}

// Exchanged state rows of the NS sequences of a unit (rows[q], slice order: every slice
// stored by the block that owns it) and the G x DEN_WAVES partial sums of buffer `buf`:
// first sum(q, total) for every live q (fixed order, equal in every lane), then
// f(slice position, values, initp) per position. Only live sequences are loaded (rows[q] of a sequence
// past its last frame is never read); their values are 0 in f. The partial sums load
// with the rows, so one round trip serves both.
template <bool LOC, int NS, class FS, class F>
__device__ __forceinline__ void den_consume(const DenX &X, int unit, int buf, float *const (&rows)[NS],
                                            const bool (&live)[NS], int nsl, const float *initp, FS sum, F f) {
    int tid = threadIdx.x;
    // opaque to the optimiser: the row addresses below are rebuilt every frame instead of
    // being hoisted out of the frame loop as 64-bit values
    asm volatile("" : "+v"(tid));
    const int n = nsl * 64, lane = tid & 63;
    const float *xb = X.buf + ((size_t)unit * 2 + buf) * X.G * X.blk;
    float pv[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) pv[q] = 0.0f;
    for (int i = lane; i < X.G * DEN_WAVES; i += 64) {
#pragma unroll
        for (int q = 0; q < NS; ++q)
            if (live[q]) pv[q] += x_ld<LOC>(xb, (i / DEN_WAVES) * X.blk + q * DEN_WAVES + i % DEN_WAVES);
    }
    float v[NS][DEN_MAXS], ip[DEN_MAXS];
#pragma unroll
    for (int m = 0; m < DEN_MAXS; ++m) ip[m] = initp ? initp[min(tid + m * DEN_THREADS, n - 1)] : 0.0f;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        if (live[q]) {
#pragma unroll
            for (int m = 0; m < DEN_MAXS; ++m) v[q][m] = x_ld<LOC>(rows[q], min(tid + m * DEN_THREADS, n - 1));
        } else {
#pragma unroll
            for (int m = 0; m < DEN_MAXS; ++m) v[q][m] = 0.0f;
        }
    }
#pragma unroll
    for (int q = 0; q < NS; ++q)
        if (live[q]) sum(q, wave_sum(pv[q]));
#pragma unroll
    for (int m = 0; m < DEN_MAXS; ++m) {
        const int c = tid + m * DEN_THREADS;
        if (c < n) {
            DenV<NS> val;
#pragma unroll
            for (int q = 0; q < NS; ++q) val.x[q] = v[q][m];
            f(c, val, ip[m]);
        }
    }
}

// new state values of the live sequences into the NS-interleaved LDS row (a sequence
// past its last frame keeps its final state for the end-of-launch totals)
template <int NS>
__device__ __forceinline__ void den_put(float *row, int st, const DenV<NS> &v, const bool (&live)[NS]) {
    if constexpr (NS == 2) {
        float2 *p = reinterpret_cast<float2 *>(row) + st;
        if (live[0] && live[1]) *p = make_float2(v.x[0], v.x[1]);
        else if (live[0]) row[2 * st] = v.x[0];
        else if (live[1]) row[2 * st + 1] = v.x[1];
    } else {
        if (live[0]) row[st] = v.x[0];
    }
}

// gather-sum over one slice of a SELL table for the NS sequences (fixed arc order per
// sequence). Records carry LDS byte offsets pre-scaled for the NS layout: state row at
// `sv`, exp row at `sx`.
template <int NS>
__device__ __forceinline__ void sell_slice(const uint2 *arcs, int len, int off, int lane, const unsigned char *sv,
                                           const unsigned char *sx, float (&acc)[NS]) {
#pragma clang fp contract(off)  // (a * tp) * x + acc rounded as the oracle does, any NS
    const uint2 *e = arcs + (size_t)off * 64 + lane;
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = 0.f;
    for (int k = 0; k < len; k += 8) {  // 8 records in flight per lane (len is a multiple of 8)
        uint2 rr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) rr[i] = e[(k + i) * 64];
        DenV<NS> a[8], x[8];  // all 16 gathers in flight before the first product
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a[i] = lds_v<NS>(sv, rr[i].x & 0xFFFF);
            x[i] = lds_v<NS>(sx, rr[i].x >> 16);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float tp = __uint_as_float(rr[i].y);
#pragma unroll
            for (int q = 0; q < NS; ++q) acc[q] += a[i].x[q] * tp * x[i].x[q];
        }
    }
}

// Per-block SELL state: len / off of every slice and this block's slot list (slot k is
// processed by wave k % DEN_WAVES; -1 = empty) in LDS; initp stays in global memory
// (L2-resident, read once per position per frame), which keeps the NS = 2 recursion small
// enough to share a CU with the numerator kernel on the side stream. States are named by
// slice position (make_den_tables), so no permutation is needed: positions >= S are
// padding.
struct SellLds {
    const int *len, *off;  // [nsl] each
    const int *slot;       // [spg]
    const float *initp;    // [nsl*64], global
};
__device__ __forceinline__ SellLds stage_sell(const SellDev &T, int lgG, int gi, int spg, unsigned char *base) {
    int *lenl = reinterpret_cast<int *>(base), *offl = lenl + T.nsl;
    int *slotl = offl + T.nsl;
    for (int i = threadIdx.x; i < T.nsl; i += DEN_THREADS) {
        lenl[i] = T.len[i];
        offl[i] = T.off[i];
    }
    for (int i = threadIdx.x; i < spg; i += DEN_THREADS) slotl[i] = T.slot[lgG][gi * spg + i];
    SellLds L{lenl, offl, slotl, T.initp};
    return L;
}

// The NS sequences of unit `unit` (sequence NS*unit + q; absent past nseqs) and their frame
// counts, row offsets and liveness at iteration `it` of a recursion.
template <int NS> struct DenUnit {
    int seq[NS], T[NS];
    long long r0[NS];
    bool has[NS];
    __device__ __forceinline__ DenUnit(const DenRun &r, const DenX &X, int unit) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            seq[q] = unit * NS + q;
            has[q] = unit < X.nseq && seq[q] < X.nseqs;
            T[q] = has[q] ? r.frames[seq[q]] : 0;
            r0[q] = has[q] ? r.row0[seq[q]] : 0;
        }
    }
    __device__ __forceinline__ int tmax() const {
        int m = 0;
#pragma unroll
        for (int q = 0; q < NS; ++q) m = max(m, T[q]);
        return m;
    }
};

// exp(clamp(x)) of the NS prefetched rows into the interleaved exp row; 0 for a sequence
// with no row (`on` false)
template <typename XT, int NS>
__device__ __forceinline__ void den_put_exp(float *xe, int P, const RowPre<XT> (&pre)[NS], const bool (&on)[NS]) {
#pragma unroll
    for (int i = 0; i < DEN_MAXPT; ++i) {
        const int p = threadIdx.x + i * DEN_THREADS;
        if (p < P) {
#pragma unroll
            for (int q = 0; q < NS; ++q)  // kernel_apply_exp
                xe[NS * p + q] = on[q] ? expf(fmaxf(-30.0f, fminf(30.0f, pre[q].get(i, P)))) : 0.0f;
        }
    }
}

// Forward pass (chain_den.cu:583-620), G blocks per unit: block gi computes alpha[t+1]
// for the destination rows of its slices (a load-balanced share, SellDev::slot) for the
// NS sequences and stores them into row t+1 of each sequence's alpha store, which is also
// the exchange: all blocks rebuild the full alpha'[t+1] in LDS from those rows. The store
// keeps the slices before the leaky term: alpha'[t] = row[t] + asum[t] * leaky * init,
// which k_den_post applies when it loads the row (one write per frame, not two).
template <typename XT, bool LOC, int NS>
__device__ __forceinline__ void den_fwd_body(const DenDev &g, const DenRun &r, const DenX &X,
                                             unsigned char *smem, int unit, int gi) {
    const int S = g.S, P = g.P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = X.G, nsl = g.f.nsl, spg = X.spg;
    const int PP = P + (P & 1);
    float *red = reinterpret_cast<float *>(smem);          // [32]
    int *flag = reinterpret_cast<int *>(smem) + 32;        // [32]
    const int rs = nsl * 64;  // rows (LDS and stored) are in slice order: contiguous, whole lines
    float *va = reinterpret_cast<float *>(smem) + 64;      // [rs][NS] alpha'[t]
    float *xe = va + NS * rs;                              // [PP][NS] exp(clamp(x))
    unsigned char *sbase = reinterpret_cast<unsigned char *>(xe + NS * PP);
    const unsigned char *sv = reinterpret_cast<const unsigned char *>(va);
    const unsigned char *sx = reinterpret_cast<const unsigned char *>(xe);

    const DenUnit<NS> U(r, X, unit);
    const int Tm = U.tmax();
    const XT *nnet = reinterpret_cast<const XT *>(r.nnet);
    const float leaky = r.leaky;
    float *astore[NS], *asum[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int sq = U.has[q] ? U.seq[q] : 0;
        astore[q] = r.alpha_store + (size_t)sq * (r.max_frames + 1) * rs;
        asum[q] = r.asum_store + (size_t)sq * (r.max_frames + 1);
    }
    const uint2 *arcs = g.f.arc_p[NS - 1];
    const SellLds F = stage_sell(g.f, X.lgG, gi, spg, sbase);
    float part = 0.f;
    for (int s = tid; s < S; s += DEN_THREADS) part += g.init[s];
    const float as0 = block_sum<DEN_WAVES>(part, red);  // AlphaFirstFrame + AlphaDash(0)
    float as[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) as[q] = as0;
    for (int c = tid; c < rs; c += DEN_THREADS) {
        const float ip = F.initp[c];  // init of the state at position c (0 for padding)
        const float v = ip + as0 * leaky * ip;
#pragma unroll
        for (int q = 0; q < NS; ++q) va[NS * c + q] = v;
    }
    if (gi == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            if (!U.has[q]) continue;
            for (int c = tid; c < rs; c += DEN_THREADS) __builtin_nontemporal_store(F.initp[c], astore[q] + c);
            if (tid == 0) {
                asum[q][0] = as0;
                r.stats[(size_t)U.seq[q] * 8 + 3] = 0.0f;  // accumulated by k_den_post
                r.stats[(size_t)U.seq[q] * 8 + 6] = 0.0f;
            }
        }
    }
    RowPre<XT> pre[NS];
    bool on[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        on[q] = U.T[q] > 0;
        if (on[q]) pre[q].fetch(nnet + U.r0[q] * r.ld, P);
    }
    den_put_exp<XT, NS>(xe, P, pre, on);
    __syncthreads();
    const bool tr = r.trace && unit == 0 && gi == 0 && tid == 0;
#define DEN_TP(i) \
    if (tr && t >= 16 && t < 48) r.trace[(t - 16) * 8 + (i)] = wall_clock64();
    for (int t = 0; t < Tm; ++t) {
        DEN_TP(0);
        bool live[NS];
        float *arow[NS], inv[NS], pq[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            live[q] = t < U.T[q];
            arow[q] = astore[q] + (size_t)(t + 1) * rs;
            inv[q] = as[q] > 0.0f ? 1.0f / as[q] : 1.0f;
            pq[q] = 0.f;
        }
        const int buf = (t + 1) & 1;
        float *tail = X.buf + (((size_t)unit * 2 + buf) * G + gi) * X.blk;
        for (int k = wave; k < spg; k += DEN_WAVES) {
            const int j = F.slot[k];
            if (j < 0) continue;
            const bool real = j * 64 + lane < S;  // padding positions stay 0
            float acc[NS];
            sell_slice<NS>(arcs, F.len[j], F.off[j], lane, sv, sx, acc);
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const float v = real ? acc[q] * inv[q] : 0.0f;
                if (live[q]) x_st<LOC>(arow[q], j * 64 + lane, v);
                pq[q] += v;
            }
        }
        if (r.trace && unit == 0 && gi < 2 && lane == 0 && t >= 16 && t < 48)  // per-wave arc end, blocks 0, 1
            r.trace[256 + ((t - 16) * 2 + gi) * DEN_WAVES + wave] = wall_clock64();
        DEN_TP(1);
        float ws[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) ws[q] = wave_sum(pq[q]);
        den_publish<LOC, NS>(X, tail, ws, unit);
        DEN_TP(2);
        // the next frame's output rows: fetched after the publish, so their latency hides
        // under the exchange wait (fetched at the frame start, the record loads' in-order
        // vmcnt waits queue behind them)
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            on[q] = t + 1 < U.T[q];
            if (on[q]) pre[q].fetch(nnet + (U.r0[q] + (long long)(t + 1) * r.stride) * r.ld, P);
        }
        DEN_TP(3);
        if (!den_wait(X, unit, (unsigned)(G * (t + 1)), flag)) return;
        DEN_TP(4);
        float as1[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) as1[q] = as[q];
        DEN_TP(5);
        den_consume<LOC, NS>(X, unit, buf, arow, live, nsl, F.initp,
                             [&](int q, float v) { as1[q] = v; },
                             [&](int st, DenV<NS> v, float ip) {
#pragma unroll
                                 for (int q = 0; q < NS; ++q) v.x[q] += as1[q] * leaky * ip;
                                 den_put<NS>(va, st, v, live);
                             });
        DEN_TP(6);
        // past the publish barrier nothing reads this frame's xe
        den_put_exp<XT, NS>(xe, P, pre, on);
        if (gi == 0 && tid == 0) {
#pragma unroll
            for (int q = 0; q < NS; ++q)
                if (live[q]) asum[q][t + 1] = as1[q];
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) as[q] = as1[q];
        __syncthreads();
        DEN_TP(7);
    }
#undef DEN_TP
    if (gi != 0) return;
    // total_prob = sum(alpha'[T]); log_correction = sum_{t<T} log(alpha_sum[t])
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        if (!U.has[q]) continue;  // uniform
        part = 0.f;
        for (int c = tid; c < rs; c += DEN_THREADS) part += va[NS * c + q];
        const float total = block_sum<DEN_WAVES>(part, red);
        double lc = 0.0;
        for (int t = tid; t < U.T[q]; t += DEN_THREADS) {
            float a = asum[q][t];
            if (a > 0.0f) lc += log((double)a);
        }
        double *redd = reinterpret_cast<double *>(smem) + 8;  // red[16..31]
        __syncthreads();
        lc = block_sum_d<DEN_WAVES>(lc, redd);
        if (tid == 0) {
            const int sq = U.seq[q];
            r.den_out[sq * 2 + 0] = total;
            r.den_out[sq * 2 + 1] = (float)(log((double)total) + lc);
            r.stats[(size_t)sq * 8 + 1] = r.den_out[sq * 2 + 1];
        }
        __syncthreads();
    }
}
template <typename XT, int NS>
__global__ __launch_bounds__(DEN_THREADS) void k_den_fwd(const DenDev g, const DenRun r, const DenX X) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int unit, gi;
    den_map(X, unit, gi);
    const int loc = den_xcd_local(X, unit, reinterpret_cast<int *>(smem) + 32);
    if (loc > 0) den_fwd_body<XT, true, NS>(g, r, X, smem, unit, gi);
    else if (loc == 0) den_fwd_body<XT, false, NS>(g, r, X, smem, unit, gi);
}

// Backward recursion (chain_den.cu:632-684 without the posteriors), G blocks per unit:
// beta'[t] over the source rows of this block's slices for the NS sequences, stored into
// row t of each sequence's beta store, which is also the exchange; beta[t] = beta'[t] +
// leaky*<init, beta'[t]>, the second term kept per frame in bsum (k_den_post adds it).
// The reference scales beta'[t] by 1/sum(alpha[t]) and starts from 1/total_prob; any
// positive per-frame factor gives the same posteriors once k_den_post normalises each
// frame (the den posteriors of a frame sum to one: they are d log p / d x_t), so this
// pass scales by 1/<init, beta'[t+1]> and starts from ones — it needs nothing from the
// forward pass and runs beside it. Iteration `it` is frame T_q - 1 - it of sequence q.
template <typename XT, bool LOC, int NS>
__device__ __forceinline__ void den_bwd_body(const DenDev &g, const DenRun &r, const DenX &X,
                                             unsigned char *smem, int unit, int gi) {
    const int S = g.S, P = g.P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = X.G, nsl = g.b.nsl, spg = X.spg;
    const int PP = P + (P & 1);
    float *red = reinterpret_cast<float *>(smem);      // [32]
    int *flag = reinterpret_cast<int *>(smem) + 32;    // [32]
    const int rs = nsl * 64;
    float *vb = reinterpret_cast<float *>(smem) + 64;  // [rs][NS] beta[t+1], slice order
    float *xe = vb + NS * rs;                          // [PP][NS] exp(clamp(x))
    unsigned char *sbase = reinterpret_cast<unsigned char *>(xe + NS * PP);
    const unsigned char *sv = reinterpret_cast<const unsigned char *>(vb);
    const unsigned char *sx = reinterpret_cast<const unsigned char *>(xe);

    const DenUnit<NS> U(r, X, unit);
    const int Tm = U.tmax();
    const XT *nnet = reinterpret_cast<const XT *>(r.nnet);
    const float leaky = r.leaky;
    float *bstore[NS], *bsum[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int sq = U.has[q] ? U.seq[q] : 0;
        bstore[q] = r.beta_store + (size_t)sq * (r.max_frames + 1) * rs;
        bsum[q] = r.bsum_store + (size_t)sq * (r.max_frames + 1);
    }
    const uint2 *arcs = g.b.arc_p[NS - 1];
    const SellLds B = stage_sell(g.b, X.lgG, gi, spg, sbase);
    // BetaDashLastFrame up to the per-frame factor: beta'[T] = 1, <init, 1> = sum(init)
    float part = 0.f;
    for (int s = tid; s < S; s += DEN_THREADS) part += g.init[s];
    const float n0 = block_sum<DEN_WAVES>(part, red);
    float nrm[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) nrm[q] = n0;
    for (int c = tid; c < rs; c += DEN_THREADS) {
#pragma unroll
        for (int q = 0; q < NS; ++q) vb[NS * c + q] = 1.0f + leaky * n0;
    }
    if (gi == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            if (!U.has[q]) continue;
            float *bT = bstore[q] + (size_t)U.T[q] * rs;
            for (int c = tid; c < rs; c += DEN_THREADS) __builtin_nontemporal_store(1.0f, bT + c);
            if (tid == 0) bsum[q][U.T[q]] = n0;
        }
    }
    RowPre<XT> pre[NS];
    bool on[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        on[q] = U.T[q] > 0;
        if (on[q]) pre[q].fetch(nnet + (U.r0[q] + (long long)(U.T[q] - 1) * r.stride) * r.ld, P);
    }
    den_put_exp<XT, NS>(xe, P, pre, on);
    __syncthreads();
    for (int it = 0; it < Tm; ++it) {
        bool live[NS];
        int tq[NS];
        float *brow[NS], inv[NS], pq[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            tq[q] = U.T[q] - 1 - it;
            live[q] = tq[q] >= 0;
            brow[q] = bstore[q] + (size_t)max(tq[q], 0) * rs;
            inv[q] = nrm[q] > 0.0f ? 1.0f / nrm[q] : 1.0f;
            pq[q] = 0.f;
        }
        const int buf = it & 1;
        float *tail = X.buf + (((size_t)unit * 2 + buf) * G + gi) * X.blk;
        for (int k = wave; k < spg; k += DEN_WAVES) {  // kernel_den_backward_transitions
            const int j = B.slot[k];
            if (j < 0) continue;
            const bool real = j * 64 + lane < S;  // padding positions stay 0
            const float ip = B.initp[j * 64 + lane];
            float acc[NS];
            sell_slice<NS>(arcs, B.len[j], B.off[j], lane, sv, sx, acc);
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const float bd = real ? acc[q] * inv[q] : 0.0f;
                if (live[q]) x_st<LOC>(brow[q], j * 64 + lane, bd);
                pq[q] += ip * bd;
            }
        }
        float ws[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) ws[q] = wave_sum(pq[q]);
        den_publish<LOC, NS>(X, tail, ws, unit);
#pragma unroll
        for (int q = 0; q < NS; ++q) {  // as den_fwd_body
            on[q] = tq[q] > 0;
            if (on[q]) pre[q].fetch(nnet + (U.r0[q] + (long long)(tq[q] - 1) * r.stride) * r.ld, P);
        }
        if (!den_wait(X, unit, (unsigned)(G * (it + 1)), flag)) return;
        float tb[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) tb[q] = 0.f;
        den_consume<LOC, NS>(X, unit, buf, brow, live, nsl, nullptr,
                             [&](int q, float v) {
                                 nrm[q] = v;  // <init, beta'[t]>: the next factor
                                 tb[q] = leaky * v;
                             },
                             [&](int st, DenV<NS> v, float) {
#pragma unroll
                                 for (int q = 0; q < NS; ++q) v.x[q] += tb[q];
                                 den_put<NS>(vb, st, v, live);
                             });
        if (gi == 0 && tid == 0) {
#pragma unroll
            for (int q = 0; q < NS; ++q)
                if (live[q]) bsum[q][tq[q]] = nrm[q];
        }
        den_put_exp<XT, NS>(xe, P, pre, on);
        __syncthreads();
    }
}

// Forward and backward recursions of every unit in one launch: blocks of the first half
// run alpha with exchange XF, the second half beta with XB (the two passes are
// independent, see den_bwd_body). One launch keeps all 2*units*G blocks co-resident,
// which the bounded exchange polls rely on; the XCD grouping of den_map is kept (G
// consecutive ids share an XCD).
template <typename XT, int NS>
__global__ __launch_bounds__(DEN_THREADS) void k_den_fb(const DenDev g, const DenRun r, const DenX XF,
                                                        const DenX XB) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the numerator kernel's waves share some of these CUs (side stream, it has ~2 ms of
    // slack under this launch): the recursion's waves win the issue arbitration
    __builtin_amdgcn_s_setprio(3);
    const int half = XF.nseq * XF.G, nb = 2 * half, b = blockIdx.x;
    int w = b;
    if (nb % 8 == 0 && (nb / 8) % XF.G == 0) w = (b % 8) * (nb / 8) + b / 8;
    const bool bwd = w >= half;
    const int inner = bwd ? w - half : w;
    const int unit = inner >> XF.lgG, gi = inner & (XF.G - 1);
    const int loc = den_xcd_local(bwd ? XB : XF, unit, reinterpret_cast<int *>(smem) + 32);
    if (loc < 0) return;  // timed out (reported through the timeout words)
    if (bwd) {
        if (loc) den_bwd_body<XT, true, NS>(g, r, XB, smem, unit, gi);
        else den_bwd_body<XT, false, NS>(g, r, XB, smem, unit, gi);
    } else {
        if (loc) den_fwd_body<XT, true, NS>(g, r, XF, smem, unit, gi);
        else den_fwd_body<XT, false, NS>(g, r, XF, smem, unit, gi);
    }
}

// Posteriors (kernel_den_posteriors, chain_den.cu:253-280) for every (sequence,
// frame) in parallel — gamma[t] needs only the stored alpha'[t] and beta[t+1] — by
// pdf rows in arc order (no atomics), and in the product mode the objective
// assembly of backward.go:224-371 into the fp16 gradient row. The whole pass always
// runs; a non-finite objective only zeroes what is written. PAIR frames share one
// stream of the pdf-ordered arc records (the pass is bound by that L2 stream).
#define POST_FRAMES 2  // frames per block (one two-frame pass: 1.82 -> 1.76 ms against 4)
// records carry LDS byte offsets into the PAIR-interleaved alpha' / beta rows (one
// 8-byte gather per operand serves both frames)
template <int PAIR>
__device__ __forceinline__ void post_slice(const uint2 *arcs, int len, int off, int lane,
                                           const unsigned char *sva, const unsigned char *svb, float acc[PAIR]) {
#pragma clang fp contract(off)  // (alpha * tp) * beta + acc, as the oracle rounds
    const uint2 *e = arcs + (size_t)off * 64 + lane;
#pragma unroll
    for (int f = 0; f < PAIR; ++f) acc[f] = 0.f;
    // (16 records in flight instead of 8: 1738 -> 1812 us per launch, r5)
    for (int k = 0; k < len; k += 8) {
        uint2 rr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) rr[i] = e[(k + i) * 64];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const DenV<PAIR> a = lds_v<PAIR>(sva, rr[i].x & 0xFFFF), b = lds_v<PAIR>(svb, rr[i].x >> 16);
            const float tp = __uint_as_float(rr[i].y);
#pragma unroll
            for (int f = 0; f < PAIR; ++f) acc[f] += a.x[f] * tp * b.x[f];
        }
    }
}
template <typename XT, int MODE, int PAIR>
__global__ __launch_bounds__(DEN_THREADS) void k_den_post(const DenDev g, const DenRun r, int nfb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int S = g.S, P = g.P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seq = blockIdx.x / nfb, fb = blockIdx.x % nfb;
    const int nslq = g.q.nsl;
    const int rsf = g.f.nsl * 64, rsb = g.b.nsl * 64;  // slice-ordered rows (k_den_fb)
    float *red = reinterpret_cast<float *>(smem);      // [32]
    float *va = reinterpret_cast<float *>(smem) + 64;  // [rsf][PAIR] alpha'[t+f], f-table slice order
    float *vb = va + PAIR * rsf;                       // [rsb][PAIR] beta[t+f+1], b-table slice order
    float *gam = vb + PAIR * rsb;                      // [PAIR][P] den, then the gradient
    int *metaq = reinterpret_cast<int *>(gam + PAIR * P);
    const int *permq = metaq, *lenq = metaq + nslq * 64, *offq = metaq + nslq * 65;
    for (int i = tid; i < nslq * 64; i += DEN_THREADS) metaq[i] = g.q.perm[i];
    for (int i = tid; i < nslq; i += DEN_THREADS) {
        metaq[nslq * 64 + i] = g.q.len[i];
        metaq[nslq * 65 + i] = g.q.off[i];
    }

    const int T = r.frames[seq];
    const int t0 = fb * POST_FRAMES, t1 = min(T, t0 + POST_FRAMES);
    // a sequence without frames adds nothing to kf_chain_result (its statistics would
    // otherwise be those of the sequence an earlier compute ran in this slot)
    if (MODE == DEN_PRODUCT && T <= 0 && fb == 0 && tid < 8) r.stats[(size_t)seq * 8 + tid] = 0.0f;
    if (t0 >= t1) return;
    const long long row0 = r.row0[seq];
    const XT *nnet = reinterpret_cast<const XT *>(r.nnet);
    const float *astore = r.alpha_store + (size_t)seq * (r.max_frames + 1) * rsf;
    const float *bstore = r.beta_store + (size_t)seq * (r.max_frames + 1) * rsb;
    const float *asum = r.asum_store + (size_t)seq * (r.max_frames + 1);
    const float *bsum = r.bsum_store + (size_t)seq * (r.max_frames + 1);
    const float leaky = r.leaky;

    int ok = 1;
    float w = 1.0f;
    const LogFstDev *nf = nullptr;
    int NG = 0;
    if (MODE == DEN_PRODUCT) {
        nf = &r.nums[seq];
        NG = nf->G;
        w = r.opts.supervision_weight;
        if (r.seq_w) w *= r.seq_w[seq];  // w_i, block-uniform
        const float num_lp = *nf->total;
        const float den_lp = r.den_out[seq * 2 + 1];
        double objf = (double)w * ((double)num_lp - (double)den_lp);
        ok = !(isnan(objf) || isinf(objf));
        if (fb == 0 && tid == 0) {
            float *st8 = r.stats + (size_t)seq * 8;
            st8[0] = num_lp;
            st8[1] = den_lp;
            st8[2] = ok ? (float)objf : (float)(-10.0 * w * T);  // backward.go:356-363
            st8[4] = w * (float)T;
            st8[5] = (float)T;
            st8[7] = ok ? 1.0f : 0.0f;
        }
    }
    const float l2s = w * r.opts.l2_regularize;
    const float oscale = 2.0f * r.opts.out_of_range_regularize;
    const bool do_oor = MODE == DEN_PRODUCT && r.opts.out_of_range_regularize > 0.0f;
    const bool do_l2 = MODE == DEN_PRODUCT && r.opts.l2_regularize > 0.0f;
    float oor = 0.f, sq = 0.f;
    // this thread's positions c = tid + m * DEN_THREADS of the alpha' rows: the initial
    // probability, once for the block's frames (rs <= DEN_MAXS * DEN_THREADS); the rows
    // are copied to LDS position for position (the records name slice positions)
    float ipf[DEN_MAXS];
#pragma unroll
    for (int m = 0; m < DEN_MAXS; ++m) {
        const int c = tid + m * DEN_THREADS;
        ipf[m] = c < rsf ? g.f.initp[c] : 0.f;
    }
    for (int t = t0; t < t1; t += PAIR) {
        const int nf2 = min(PAIR, t1 - t);
        // stage alpha'[t+f], beta[t+f+1] (a missing second frame computes zeros); the
        // stored rows lack the leaky terms (den_fwd_body, den_bwd_body), added here as the
        // recursions add them
        // both frames' rows are loaded before the first LDS store, which then writes each
        // position's PAIR values as one vector (a PAIR-strided scalar store is 2-way conflicted)
        float va_[PAIR][DEN_MAXS], vb_[PAIR][DEN_MAXS], as1[PAIR], tb[PAIR];
#pragma unroll
        for (int f = 0; f < PAIR; ++f) {
            const bool live = f < nf2;
            // (a missing frame reads frame t's rows, which exist, and stores zeros)
            const int tf = live ? t + f : t;
            const float *ar = astore + (size_t)tf * rsf, *br = bstore + (size_t)(tf + 1) * rsb;
            as1[f] = live ? asum[t + f] : 0.f;
            tb[f] = live ? leaky * bsum[t + f + 1] : 0.f;
#pragma unroll
            for (int m = 0; m < DEN_MAXS; ++m) {  // unconditional loads (index clamped)
                const int c = tid + m * DEN_THREADS;
                va_[f][m] = __builtin_nontemporal_load(ar + min(c, rsf - 1));
                vb_[f][m] = __builtin_nontemporal_load(br + min(c, rsb - 1));
            }
        }
#pragma unroll
        for (int m = 0; m < DEN_MAXS; ++m) {
            const int c = tid + m * DEN_THREADS;
            DenV<PAIR> a, b;
#pragma unroll
            for (int f = 0; f < PAIR; ++f) {
                const bool live = f < nf2;
                a.x[f] = live ? va_[f][m] + as1[f] * leaky * ipf[m] : 0.f;
                b.x[f] = live ? vb_[f][m] + tb[f] : 0.f;
            }
            if constexpr (PAIR == 2) {
                if (c < rsf) reinterpret_cast<float2 *>(va)[c] = make_float2(a.x[0], a.x[1]);
                if (c < rsb) reinterpret_cast<float2 *>(vb)[c] = make_float2(b.x[0], b.x[1]);
            } else {
                if (c < rsf) va[c] = a.x[0];
                if (c < rsb) vb[c] = b.x[0];
            }
        }
        __syncthreads();
        float gpart[PAIR];
#pragma unroll
        for (int f = 0; f < PAIR; ++f) gpart[f] = 0.f;
        for (int k = wave; k < g.q.spg[0]; k += DEN_WAVES) {
            const int j = g.q.slot[0][k];
            if (j < 0) continue;
            const int pdf = permq[j * 64 + lane];
            float acc[PAIR];
            post_slice<PAIR>(g.q.arc_p[PAIR - 1], lenq[j], offq[j], lane, reinterpret_cast<const unsigned char *>(va),
                             reinterpret_cast<const unsigned char *>(vb), acc);
            if (pdf < 0) continue;
#pragma unroll
            for (int f = 0; f < PAIR; ++f) {
                if (f >= nf2) break;
                const float x = (float)nnet[(row0 + (long long)(t + f) * r.stride) * r.ld + pdf];
                const float gv = acc[f] * expf(fmaxf(-30.0f, fminf(30.0f, x)));  // kernel_apply_exp
                gam[f * P + pdf] = gv;
                gpart[f] += gv;
            }
        }
#pragma unroll
        for (int f = 0; f < PAIR; ++f) {
            if (f >= nf2) break;
            const int tf = t + f;
            // the frame's occupation sums to one (alpha and beta carry arbitrary
            // per-frame factors, see den_bwd_body): normalise in a fixed order
            const float gsum = block_sum<DEN_WAVES>(gpart[f], red);
            const float ginv = gsum > 0.0f ? 1.0f / gsum : 0.0f;
            float *gm = gam + f * P;
            if (MODE == DEN_ABI) {
                for (int pdf = tid; pdf < P; pdf += DEN_THREADS)
                    r.post_dense[(size_t)tf * P + pdf] = gm[pdf] * ginv;
            } else {
                // d = (oor) + w*num - w*den - l2: -w*den first, the numerator's sparse
                // posteriors (its pdf set) added in place, then the dense pass
                for (int pdf = tid; pdf < P; pdf += DEN_THREADS) gm[pdf] = -(w * (gm[pdf] * ginv));
                __syncthreads();
                const float *nps = nf->post_sparse + (size_t)tf * NG;
                for (int q = tid; q < NG; q += DEN_THREADS) {
                    const int p = nf->grp_pdf[q];
                    if (p > 0 && p <= P) gm[p - 1] = w * nps[q] + gm[p - 1];
                }
                __syncthreads();
                const XT *xrow = nnet + (row0 + (long long)tf * r.stride) * r.ld;
                h16 *orow = r.out_grad + (row0 + (long long)tf * r.stride) * r.ldg;
                const bool even = (tf & 1) == 0;
                // the frame's deriv weight, one block-uniform load (Kaldi's MulRowsVec, after
                // every term is in): one fp32 multiply, then the one rounding
                // (the loss scale, DESIGN §30: one more block-uniform load beside it)
                float fw = r.frame_w ? r.frame_w[(size_t)seq * r.max_frames + tf] : 1.0f;
                if (r.grad_scale) fw *= *r.grad_scale;
                for (int pdf = tid; pdf < P; pdf += DEN_THREADS) {
                    const float x = (float)xrow[pdf];
                    float d = 0.0f;
                    if (do_oor && even) {  // chain_backward.cu:27-67
                        if (x < -30.0f) {
                            d += (-30.0f - x) * oscale;
                            oor += 1.0f;
                        } else if (x > 30.0f) {
                            d += (30.0f - x) * oscale;
                            oor += 1.0f;
                        }
                    }
                    d += gm[pdf];
                    if (do_l2) {
                        d -= l2s * x;
                        sq += x * x;
                    }
                    orow[pdf] = ok ? (h16)(-(d * fw)) : (h16)0.0f;  // loss gradient = -deriv
                }
            }
            __syncthreads();
        }
    }
    if (MODE == DEN_PRODUCT) {
        float o = block_sum<DEN_WAVES>(oor, red);
        __syncthreads();
        float q = block_sum<DEN_WAVES>(sq, red);
        if (tid == 0) {
            float *st8 = r.stats + (size_t)seq * 8;
            if (o > 0.0f) atomicAdd(&st8[6], o);
            if (do_l2 && ok) atomicAdd(&st8[3], -0.5f * l2s * q);
        }
    }
}

// initp[c] = init[perm[c]] (0 for padding rows): the initial probabilities in a
// SELL table's slice order, so the exchange consumers load them with the payload
__global__ void k_perm_gather(const int *perm, const float *init, float *out, int n) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) out[c] = perm[c] >= 0 ? init[perm[c]] : 0.0f;
}

// ===========================================================================
// Host: device tables of a graph, exchange sizing, launches
// ===========================================================================
static_assert(sizeof(SellRec) == sizeof(uint2), "SellRec is uploaded as the kernels' uint2");

DenTables *make_den_tables(int S, int P, int A, const int32_t *src, const int32_t *dst,
                           const int32_t *pdf0, const float *tp, const char **why) {
    DenHost h;
    if (!den_host_tables(S, P, A, src, dst, pdf0, tp, h, why)) return nullptr;
    auto *t = new DenTables();
    DenDev &d = t->dev;
    d.S = S;
    d.P = P;
    bool ok = true;
    auto put = [&](SellDev &o, const DenHostTable &ht) {
        o.nsl = (int)ht.sell.len.size();
        o.perm = dev_upload(ht.sell.perm, t->owned);
        o.len = dev_upload(ht.sell.len, t->owned);
        o.off = dev_upload(ht.sell.off, t->owned);
        ok = ok && o.perm && o.len && o.off;
        for (int lg = 0; lg < 4; ++lg) {
            o.slot[lg] = nullptr;
            o.spg[lg] = ht.spg[lg];
            if (ht.slot[lg].empty()) continue;
            o.slot[lg] = dev_upload(ht.slot[lg], t->owned);
            ok = ok && o.slot[lg];
        }
    };
    put(d.f, h.f);
    put(d.b, h.b);
    put(d.q, h.q);
    d.pair_ok = h.pair_ok;
    auto scaled = [&](const Sell &sl, uint32_t ns) {
        return reinterpret_cast<const uint2 *>(dev_upload(sell_scaled(sl, ns), t->owned));
    };
    for (int ns = 1; ns <= 2; ++ns) {
        d.f.arc_p[ns - 1] = scaled(h.f.sell, ns);
        d.b.arc_p[ns - 1] = scaled(h.b.sell, ns);
        d.q.arc_p[ns - 1] = scaled(h.q.sell, ns);
        ok = ok && d.f.arc_p[ns - 1] && d.b.arc_p[ns - 1] && d.q.arc_p[ns - 1];
    }
    std::vector<float> zf(h.f.sell.perm.size(), 0.0f), zb(h.b.sell.perm.size(), 0.0f);
    d.f.initp = dev_upload(zf, t->owned);  // filled by den_tables_set_init
    d.b.initp = dev_upload(zb, t->owned);
    ok = ok && d.f.initp && d.b.initp;
    if (!ok) {
        delete t;
        *why = "hipMalloc failed for den tables";
        return nullptr;
    }
    return t;
}

// (re)derive the slice-ordered initial probabilities from a device init vector
void den_tables_set_init(const DenDev &d, const float *d_init, hipStream_t st) {
    const int nf = d.f.nsl * 64, nb = d.b.nsl * 64;
    hipLaunchKernelGGL(k_perm_gather, dim3((nf + 255) / 256), dim3(256), 0, st, d.f.perm, d_init,
                       (float *)d.f.initp, nf);
    hipLaunchKernelGGL(k_perm_gather, dim3((nb + 255) / 256), dim3(256), 0, st, d.b.perm, d_init,
                       (float *)d.b.initp, nb);
}

// G blocks per sequence: as many as the CUs allow (every block must be resident:
// the exchange polls are bounded, so a shortfall ends in the timeout word, not a hang)
int den_pick_G(int nseq) {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 1;
    }
    for (int G = 4; G > 1; G /= 2)
        if (nseq * G <= cus) return G;
    return 1;
}

void launch_den_fwd(const DenDev &g, const DenRun &r, const DenX &X, DenXBuf &xb, bool fp32_in) {
    size_t lds = X.lds_f;
    hipStream_t st = kf_stream();
    xb.zero(st);
    dim3 grid(X.nseq * X.G);
    if (fp32_in)  // the den ABI: one sequence (X.ns == 1)
        hipLaunchKernelGGL((k_den_fwd<float, 1>), grid, dim3(DEN_THREADS), lds, st, g, r, X);
    else if (X.ns == 2)
        hipLaunchKernelGGL((k_den_fwd<h16, 2>), grid, dim3(DEN_THREADS), lds, st, g, r, X);
    else
        hipLaunchKernelGGL((k_den_fwd<h16, 1>), grid, dim3(DEN_THREADS), lds, st, g, r, X);
}
// both recursions in one launch (k_den_fb); XF / XB from two exchange buffers
void launch_den_fb(const DenDev &g, const DenRun &r, const DenX &XF, DenXBuf &xf, const DenX &XB,
                   DenXBuf &xbb, bool fp32_in) {
    hipStream_t st = kf_stream();
    xf.zero(st);
    xbb.zero(st);
    dim3 grid(2 * XF.nseq * XF.G);
    const size_t lds = std::max(XF.lds_f, XB.lds_b);
    if (fp32_in) hipLaunchKernelGGL((k_den_fb<float, 1>), grid, dim3(DEN_THREADS), lds, st, g, r, XF, XB);
    else if (XF.ns == 2) hipLaunchKernelGGL((k_den_fb<h16, 2>), grid, dim3(DEN_THREADS), lds, st, g, r, XF, XB);
    else hipLaunchKernelGGL((k_den_fb<h16, 1>), grid, dim3(DEN_THREADS), lds, st, g, r, XF, XB);
}
void launch_den_post(const DenDev &g, const DenRun &r, const DenX &X, bool fp32_in, int mode) {
    hipStream_t st = kf_stream();
    const int nfb = (r.max_frames + POST_FRAMES - 1) / POST_FRAMES;
    dim3 pgrid(X.nseqs * nfb);  // per sequence
    // frame pairs share the arc stream when both frames' alpha/beta fit in LDS
    const int rs = g.f.nsl * 64;  // = g.b.nsl * 64
    const bool pair = den_post_lds_bytes(rs, g.P, g.q.nsl, 2) <= DEN_LDS_TOTAL;
    size_t plds = den_post_lds_bytes(rs, g.P, g.q.nsl, pair ? 2 : 1);
#define KF_POST(XT_, MODE_, PAIR_) \
    hipLaunchKernelGGL((k_den_post<XT_, MODE_, PAIR_>), pgrid, dim3(DEN_THREADS), plds, st, g, r, nfb)
    if (mode == DEN_PRODUCT) {
        if (pair) KF_POST(h16, DEN_PRODUCT, 2);
        else KF_POST(h16, DEN_PRODUCT, 1);
    } else if (fp32_in) {
        if (pair) KF_POST(float, DEN_ABI, 2);
        else KF_POST(float, DEN_ABI, 1);
    } else {
        if (pair) KF_POST(h16, DEN_ABI, 2);
        else KF_POST(h16, DEN_ABI, 1);
    }
#undef KF_POST
}
