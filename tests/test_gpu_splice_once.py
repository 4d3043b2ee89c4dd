"""The single-staging kernel for two-part spliced A operands (csrc/splice_once.hip): the long-K
N = 160 / 320 products of a TDNN-F layer (linear forward, affine input gradient) with the source
rows staged in LDS once per 64-column chunk. Every case runs the same product on the new kernel
and, through kf_gemm_debug_splice_once(0), on the tiled kernel: all outputs must be identical
bit for bit (same MFMAs, same operands, same order), and both must match a float32 numpy
product of the fp16 inputs. Shapes are the smallest that reach the kernel's boundaries: row
tiles of 128, 128, 44 (M = 300), a one-row last tile (M = 129), an exact tile (M = 128), 8
chunks (pw = 512: more chunks than images in the ring, so the ring wraps), offsets 1 and 3,
clamped and zero rows in the first and last tiles, edge rows, the scratch row, N = 320.

Element bound (gemm_ref.py, the bound tests/test_gpu_gemm_tiles.py holds fused products to):
fp32 accumulation of K terms errs by at most K * 2^-23 * sum|a||b|, the epilogue adds 1e-6 |v|,
the stored fp16 one rounding |v| * 2^-10 + 2^-24. The float32 numpy reference accumulates in
fp32 itself, which adds its own K * 2^-24 * sum|a||b|.

The plan tests at the end need no GPU: kf_splice_once_debug_plan makes no HIP call."""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as gr

KF_ZERO, KF_CLAMP = 0, 1
PW = 512
SENTINEL = 0x7BFF  # 65504: rows the kernel must not touch keep it


def _fill(kf, rows, N):
    return kf.upload_fp16(np.full((rows, N), SENTINEL, np.uint16).view(np.float16))


def _raw(kf, buf, rows, N):
    return kf.read_fp16(buf.ptr, (rows, N)).view(np.uint16)


def _tol(acc, mag, K):
    return K * (2.0 ** -23 + 2.0 ** -24) * mag + 1e-6 * np.abs(acc) + np.abs(acc) * 2.0 ** -10 + 2.0 ** -24


def _within(got, ref, tol, what):
    bad = ~(np.abs(got.astype(np.float64) - ref) <= tol)  # a NaN fails
    assert not bad.any(), "%s: %d elements out of bound, worst excess %.3g" % (
        what, int(bad.sum()), float(np.nanmax(np.abs(got.astype(np.float64) - ref) - tol)))


def _both(kf, run):
    """run() on the single-staging kernel, then on the tiled kernel; the two results"""
    res = []
    try:
        for on in (1, 0):
            kf.core.kf_gemm_debug_splice_once(on)
            res.append(run())
            assert kf.splice_once_last()["taken"] == on, "hook %d: the dispatcher took the other kernel" % on
    finally:
        kf.core.kf_gemm_debug_splice_once(1)
    return res


def _forward(kf, M, N, s, edges, seed):
    """linear forward form: A = [x(t - s) | x(t)] clamped, B = W[K][N], epilogue out only"""
    K = 2 * PW
    rng = np.random.default_rng(seed)
    x = gr.h16(rng.standard_normal((M, PW)) * 0.5)
    w = gr.h16(rng.standard_normal((K, N)) / np.sqrt(K))
    dx, dw = kf.upload_fp16(x), kf.upload_fp16(w)
    A = kf.operand(dx.ptr, PW, M, K, 1, nparts=2, part_width=PW, T=M, tpolicy=KF_CLAMP, dt=(-s, 0), edges=edges)
    B = kf.operand(dw.ptr, N, K, N, 0)

    def run():
        out = _fill(kf, M + 2, N)
        E = kf.KfEpilogue(out=out.ptr, ldo=N, alpha=1.0)
        kf.check(kf.core.kf_gemm_fused(M, N, K, C.byref(A), C.byref(B), C.byref(E)), "forward form")
        kf.sync()
        return _raw(kf, out, M + 2, N)

    new, old = _both(kf, run)
    assert np.array_equal(new, old), "forward form: %d elements differ from the tiled kernel" % int((new != old).sum())
    assert (new[M:] == SENTINEL).all()
    a32 = gr.splice(x, np.arange(M), (-s, 0), KF_CLAMP, edges).astype(np.float32)
    w32 = w.astype(np.float32)
    acc, mag = (a32 @ w32).astype(np.float64), (np.abs(a32) @ np.abs(w32)).astype(np.float64)
    _within(new[:M].view(np.float16), acc, _tol(acc, mag, K), "forward form")
    return new


def _gradient(kf, M, N, s, seed):
    """affine input gradient form: A = [dz(t) | dz(t - s)] zero-padded, row M - 1 of part 1 reading
    the spare row M; B = op_wrows (B'[n][(p, k)] = W[p * N + n][k]); out2 through a row mask that
    zeroes one row; edge_out = the sum of out2's rows 0 .. s"""
    K = 2 * PW
    rng = np.random.default_rng(seed)
    x = gr.h16(rng.standard_normal((M + 1, PW)) * 0.5)
    w = gr.h16(rng.standard_normal((2 * N, PW)) / np.sqrt(K))
    zr = M // 2
    bits = np.ones((M, N), bool)
    bits[zr] = False
    mk = gr.pack_bits(bits, N)
    mk = np.concatenate([mk, np.zeros((-len(mk)) % 4, np.uint8)])
    dx, dw = kf.upload_fp16(x), kf.upload_fp16(w)
    dmk = kf.DeviceBuffer(mk.nbytes)
    kf.check(kf.core.bridge_transfer_int32(dmk.ptr, mk.ctypes.data, mk.nbytes // 4), "mask")
    edges = ((1, M - 1, M),)
    A = kf.operand(dx.ptr, PW, M, K, 1, nparts=2, part_width=PW, T=M, tpolicy=KF_ZERO, dt=(0, -s), edges=edges)
    B = kf.operand(dw.ptr, PW, N, K, 1, nparts=2, part_width=PW, T=2 * N, dt=(0, N))

    def run():
        out2 = _fill(kf, M + 2, N)
        E = kf.KfEpilogue(alpha=1.0, out2=out2.ptr, ldo2=N, mask_in=dmk.ptr, edge_out=out2.ptr + M * N * 2,
                          edge_r0=0, edge_r1=s + 1, edge_src=1)
        kf.check(kf.core.kf_gemm_fused(M, N, K, C.byref(A), C.byref(B), C.byref(E)), "gradient form")
        kf.sync()
        return _raw(kf, out2, M + 2, N)

    new, old = _both(kf, run)
    assert np.array_equal(new, old), "gradient form: %d elements differ from the tiled kernel" % int((new != old).sum())
    assert (new[M + 1] == SENTINEL).all()
    a32 = gr.splice(x, np.arange(M), (0, -s), KF_ZERO, edges).astype(np.float32)
    w32 = np.concatenate([w[:N], w[N:]], 1).astype(np.float32).T  # [K x N]
    acc, mag = (a32 @ w32).astype(np.float64), (np.abs(a32) @ np.abs(w32)).astype(np.float64)
    acc[zr] = 0.0
    got = new[:M].view(np.float16)
    _within(got, acc, _tol(acc, mag, K) * bits, "gradient form")
    assert (new[zr] == 0).all()
    # the edge row: the stored rows 0 .. s summed in row order in fp32, one rounding
    e = np.zeros(N, np.float32)
    for r in range(s + 1):
        e = e + got[r].astype(np.float32)
    assert np.array_equal(new[M], e.astype(np.float16).view(np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1, 3])
def test_forward_form(gpu, s):
    _forward(gpu, 300, 160, s, (), 11 + s)


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1, 3])
def test_forward_form_scratch_row(gpu, s):
    """the row-subsampled stack's scratch row: both parts of row 200 read the last row's inputs,
    so row 200 is row M - 1 bit for bit"""
    M = 300
    new = _forward(gpu, M, 160, s, ((0, 200, M - 1 - s), (1, 200, M - 1)), 21 + s)
    assert np.array_equal(new[200], new[M - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1, 3])
def test_gradient_form(gpu, s):
    _gradient(gpu, 300, 160, s, 31 + s)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [129, 128])
def test_ragged(gpu, M):
    """a one-row last tile and an exact tile, s = 3: the clamped (forward form) and the zero rows
    (gradient form) of the first and last tiles"""
    _forward(gpu, M, 160, 3, (), 41 + M)
    _gradient(gpu, M, 160, 3, 51 + M)


@pytest.mark.gpu
def test_n320(gpu):
    _forward(gpu, 300, 320, 3, (), 61)


# ---------------------------------------------------------------- the plan (no GPU)
def _plan(M, N, pw, dt, policy, bkc, edges=(), nparts=2, mask=None, scales=None, **epi):
    import kfp16 as kf
    K = nparts * pw
    base = 1 << 20  # never dereferenced: the plan makes no HIP call
    A = kf.operand(base, pw, M, K, 1, nparts=nparts, part_width=pw, T=M, tpolicy=policy, dt=dt, edges=edges,
                   mask=mask, mask_rows=M if mask else 0, scales=scales, lds=pw // 32 if scales else 0)
    if scales:
        B = kf.operand(base, K, N, K, 1, scales=scales, lds=K // 32)
    elif bkc:
        B = kf.operand(base, pw, N, K, 1, nparts=nparts, part_width=pw, T=nparts * N, dt=tuple(range(0, nparts * N, N)))
    else:
        B = kf.operand(base, N, K, N, 0)
    E = kf.KfEpilogue(out=base, ldo=N, alpha=1.0, **epi)
    return kf.splice_once_plan(M, N, K, A, B, E)


PLAN_CASES = [
    # M, N, pw, dt, policy, bkc, edges
    (300, 160, 512, (-1, 0), KF_CLAMP, 0, ()),
    (300, 160, 512, (-3, 0), KF_CLAMP, 0, ()),
    (300, 160, 512, (-3, 0), KF_CLAMP, 0, ((0, 200, 296), (1, 200, 299))),
    (300, 160, 512, (0, -1), KF_ZERO, 1, ((1, 299, 300),)),
    (300, 160, 512, (0, -3), KF_ZERO, 1, ((1, 299, 300),)),
    (129, 160, 512, (-3, 0), KF_CLAMP, 0, ()),
    (128, 160, 512, (0, -3), KF_ZERO, 1, ((1, 127, 128),)),
    (300, 320, 512, (-3, 0), KF_CLAMP, 0, ()),
    (32020, 160, 1536, (-1, 0), KF_CLAMP, 0, ((0, 32000, 32018), (1, 32000, 32019))),
    (32020, 160, 1536, (0, -1), KF_ZERO, 1, ((1, 32019, 32020),)),
    (96000, 160, 1536, (-3, 0), KF_CLAMP, 0, ()),
    (96000, 160, 1536, (0, -3), KF_ZERO, 1, ((1, 95999, 96000),)),
    (32020, 320, 3072, (-1, 0), KF_CLAMP, 0, ()),
    (96000, 320, 3072, (0, -3), KF_ZERO, 1, ((1, 95999, 96000),)),
]


@pytest.mark.parametrize("M,N,pw,dt,policy,bkc,edges", PLAN_CASES)
def test_plan_geometry(M, N, pw, dt, policy, bkc, edges):
    p = _plan(M, N, pw, dt, policy, bkc, edges)
    assert p["taken"] == 1
    assert (p["BM"], p["BN"]) == (128, 160)
    span = max(dt) - min(dt)
    assert p["span"] == span and p["edge_slots"] == len(edges) and p["zero_slots"] == 1
    assert p["image_rows"] == 128 + span + len(edges) + 1
    assert p["npieces"] == (p["image_rows"] + 7) // 8
    # at least two images in flight beyond the one being read, a B ring of at least two stages
    assert p["nimg"] >= 3 and p["b_stages"] >= 2
    assert p["lds"] == p["nimg"] * p["npieces"] * 1024 + p["b_stages"] * 160 * 64 * 2
    assert p["lds"] <= 160 * 1024
    assert (p["mtiles"], p["ntiles"]) == ((M + 127) // 128, N // 160)
    assert p["bkc"] == bkc


def test_plan_declines():
    ok = dict(M=300, N=160, pw=512, dt=(-3, 0), policy=KF_CLAMP, bkc=0)
    assert _plan(**ok)["taken"] == 1
    base = 1 << 20
    assert _plan(**dict(ok, policy=KF_ZERO, bkc=1, dt=(0, -3)), mask=base)["taken"] == 0       # masked A
    assert _plan(**ok, scales=base)["taken"] == 0                                              # MXFP8
    assert _plan(**ok, drop=base, ld_drop=160, row_seg=base)["taken"] == 0                    # dropout epilogue
    assert _plan(**ok, out8=base, ldo8=160, scale8=base)["taken"] == 0                        # MXFP8 copy
    assert _plan(**dict(ok, pw=256))["taken"] == 0                                             # narrow parts
    assert _plan(**dict(ok, dt=(0,)), nparts=1)["taken"] == 0                                  # single part
    assert _plan(**dict(ok, N=192))["taken"] == 0 and _plan(**dict(ok, N=480))["taken"] == 0   # other N
    assert _plan(**dict(ok, dt=(-9, 0)))["taken"] == 0                                         # |dt| > 8
