"""float64 restatement of the fused GEMM epilogue (include/kf_ops.h, KfEpilogue) and of the
weight-gradient GEMM, with the error bounds the GPU tests hold the kernels to, plus the case
tables of tests/test_gpu_gemm_tiles.py and tests/test_gpu_wgrad_tiles.py. No GPU needed:
tests/test_gemm_ref.py checks the rule and the cases' inputs from here alone.

Rule, per output element (m, n) of the fp32 accumulator acc:
  v = alpha*acc + beta*old + bias[n]
  relu:  bit = v > 0; v = max(v, 0)
  scale: v = v*scale[n] + shift[n]
  resid: v += resid_alpha * resid[m][n]
  out  = rne_fp16(v);  out2 = rne_fp16(v * scale2[n] * bit(mask_in))

Bound (the form of test_gpu_benchsize.py / test_gpu_implicit_dz.py): the fp32
accumulation of a K-term product errs by at most K * 2^-23 * sum|a||b|; the few fp32 operations
of the epilogue add 1e-6 |v| at the pre-activation. That bound decides which ReLU bits are
certain (|v| > bound) and travels through the later steps multiplied by |scale| and |scale2|
(ReLU is 1-Lipschitz; shift and the residual are added exactly in this model). A stored fp16
value adds one rounding: tol = bound + |ref| * 2^-10 + 2^-24.
Weight gradients are fp32: tol = T * 2^-23 * sum|a||b| * 1.01 + |ref| * 2^-23, times |col_scale|.
"""
import functools

import numpy as np

from mx_ref import E4M3, e4m3_encode

U23 = 2.0 ** -23
KF_ZERO, KF_CLAMP = 0, 1


def h16(a):
    return np.ascontiguousarray(a, np.float16)


# ---------------------------------------------------------------- bit masks
def pack_bits(bits, ld, pad=None):
    """bits [rows x n] -> bytes of a mask over a [rows x ld] tensor in linear element order
    (bit i of byte i / 8); the pad columns n .. ld-1 take `pad` [rows x (ld - n)] or zero"""
    bits = np.asarray(bits, bool)
    rows, n = bits.shape
    full = np.zeros((rows, ld), bool)
    full[:, :n] = bits
    if pad is not None:
        full[:, n:] = pad
    assert (rows * ld) % 8 == 0
    return np.packbits(full.reshape(-1), bitorder="little")


def unpack_bits(buf, rows, ld):
    """bytes -> bool [rows x ld] of the first rows * ld bits in linear element order"""
    b = np.unpackbits(np.asarray(buf, np.uint8), bitorder="little")[:rows * ld]
    return b.reshape(rows, ld).astype(bool)


# ---------------------------------------------------------------- operands
def splice(x, rows, dts, policy=KF_CLAMP, edges=()):
    """[x(t + dts[0]) | x(t + dts[1]) | ...] at logical rows `rows` (float64) of the first
    T = len(rows) source rows of x; out of range: clamp or zero. edges: (part, t, source row)
    triples, the part's row t reads that source row instead (kf_ops.h edge_t / edge_row)."""
    x = np.asarray(x)
    n = len(rows)
    parts = []
    for p, dt in enumerate(dts):
        idx = rows + dt
        part = x[np.clip(idx, 0, n - 1)].astype(np.float64)
        if policy != KF_CLAMP:
            part = np.where(((idx >= 0) & (idx < n))[:, None], part, 0.0)
        for pp, t, src in edges:
            if pp == p:
                part[rows == t] = x[src].astype(np.float64)
        parts.append(part)
    return np.concatenate(parts, 1)


# ---------------------------------------------------------------- epilogue
def epilogue_ref(acc, mag, K, alpha=1.0, beta=0.0, old=None, bias=None, relu=False, scale=None, shift=None,
                 resid=None, resid_alpha=0.0, scale2=None, mask_in=None):
    """acc = A @ B and mag = |A| @ |B| in float64. Returns a dict: v (the unrounded out value),
    out2 (unrounded), bits (v > 0 before the ReLU, None without one), pre (the pre-activation),
    sure (where bits are certain), bound / bound2 (on v / out2), tol / tol2 (for the stored fp16)."""
    f = np.float64
    v = f(alpha) * acc
    if beta != 0.0:
        v = v + f(beta) * old.astype(f)
    if bias is not None:
        v = v + bias.astype(f)
    pre = v
    bound = abs(alpha) * K * U23 * mag + 1e-6 * np.abs(v)
    bits = sure = None
    if relu:
        bits = v > 0
        sure = np.abs(v) > bound
        v = np.maximum(v, 0.0)
    if scale is not None:
        v = v * scale.astype(f) + shift.astype(f)
        bound = bound * np.abs(scale.astype(f))
    if resid is not None:
        v = v + f(resid_alpha) * resid.astype(f)
    out2 = v
    bound2 = bound
    if scale2 is not None:
        out2 = out2 * scale2.astype(f)
        bound2 = bound2 * np.abs(scale2.astype(f))
    if mask_in is not None:
        out2 = out2 * mask_in
        bound2 = bound2 * mask_in
    return dict(v=v, out2=out2, bits=bits, pre=pre, sure=sure, bound=bound, bound2=bound2,
                tol=bound + np.abs(v) * 2.0 ** -10 + 2.0 ** -24,
                tol2=bound2 + np.abs(out2) * 2.0 ** -10 + 2.0 ** -24)


def wgrad_tol(T, mag, acc, col_scale=None, total=None):
    """fp32 weight-gradient tolerance for acc = A^T @ B over T rows, mag = |A|^T @ |B|. With
    accumulate = 1 the stored sum old + acc (`total`) is rounded to fp32 once more."""
    tol = T * U23 * mag * 1.01 + np.abs(acc) * U23
    if col_scale is not None:
        tol = tol * np.abs(col_scale.astype(np.float64))
    if total is not None:
        tol = tol + np.abs(total) * U23
    return tol + 1e-30


# ---------------------------------------------------------------- MXFP8 copy
def _mx_exp(amax):
    _, e2 = np.frexp(amax)
    return np.clip(np.where(amax > 0, e2 - 1 - 8, 0), -126, 126).astype(np.int64)


def mx_mismatch(codes, scales, v, bound):
    """The MXFP8 copy (mx_ref.py's rule) of a value known as v +- bound: (bad scale blocks,
    bad codes) as boolean arrays. A block's scale byte must be the rule's for some amax in
    [max|v| - bound, max|v| + bound]; with the byte the kernel chose, each code must decode to
    a value between the e4m3 roundings of (v - bound) / scale and (v + bound) / scale (the
    rounding is monotone), i.e. the neighbouring code passes only within the bound of a
    rounding boundary."""
    rows, cols = v.shape
    vb, bb = v.reshape(rows, cols // 32, 32), bound.reshape(rows, cols // 32, 32)
    alo = np.maximum(np.abs(vb) - bb, 0.0).max(2)
    ahi = (np.abs(vb) + bb).max(2)
    got = scales.astype(np.int64) - 127
    ok = (got >= _mx_exp(alo)) & (got <= _mx_exp(ahi)) & (alo > 0)
    ok |= (alo == 0) & ((got == 0) | (got <= _mx_exp(ahi)))
    s = (2.0 ** got)[:, :, None]
    lo = E4M3[e4m3_encode((vb - bb) / s)]
    hi = E4M3[e4m3_encode((vb + bb) / s)]
    dec = E4M3[codes.reshape(rows, cols // 32, 32)]
    with np.errstate(invalid="ignore"):
        good = (dec >= lo) & (dec <= hi)
    return ~ok, ~good.reshape(rows, cols)


# ---------------------------------------------------------------- fused cases
# tile -> (M, N, K): the smallest shape on that tile of kf_gemm_fused's dispatch with a ragged
# last row tile, a ragged last column tile and K % 64 != 0. 128x128: 5 x 2 tiles, the XCD remap
# with remainder 2; 256x64: 9 tiles, remainder 1; 192x128: N >= 256, N % 192 != 0; 128x192:
# N % 192 == 0, K <= 640; 128x160: N = 160 with few row blocks; 384x160 needs
# ceil(M / 384) * ceil(N / 160) >= 192, so M = 95 * 384 + 10 with N = 320.
TILE_SHAPES = {
    (128, 128): (520, 200, 72),
    (256, 64): (2060, 40, 72),
    (192, 128): (200, 264, 328),
    (128, 192): (130, 384, 72),
    (128, 160): (130, 160, 72),
    (384, 160): (36490, 320, 72),
}
# the MXFP8 copy needs N % 32 == 0 and a tile whose wave tile holds whole 32-column blocks
MX_SHAPES = {(128, 128): (520, 224, 72), (256, 64): (2060, 64, 72), (192, 128): (200, 288, 328)}
EPILOGUES = ("scaled", "fwd", "bwd", "out2only", "accum")
S = 3  # splice offset


def _spliced_k(K):
    """a two-part A needs part widths that are multiples of 8: the nearest K above with
    K / 2 % 8 == 0 and K % 64 != 0"""
    K2 = (K + 15) // 16 * 16
    return K2 if K2 % 64 else K2 + 16


def fused_cases():
    """dicts: id, tile, M, N, K, epi, a ('plain' | 'clamp' | 'zero' | 'p2edge'), b ('rm' | 'kc' |
    'p2'), masked, edge (r0, r1, src) or None"""
    out = []

    def add(tile, M, N, K, epi, a="plain", b="rm", masked=False, edge=None):
        cid = "%dx%d-%dx%dx%d-%s-%s-%s" % (tile[0], tile[1], M, N, K, epi, a, b)
        if masked:
            cid += "-masked"
        if edge:
            cid += "-edge"
        out.append(dict(id=cid, tile=tile, M=M, N=N, K=K, epi=epi, a=a, b=b, masked=masked, edge=edge))

    for tile, (M, N, K) in TILE_SHAPES.items():
        for epi in EPILOGUES:
            add(tile, M, N, K, epi)
        for epi in ("fwd", "bwd"):
            add(tile, M, N, K, epi, b="kc")
        # two-part A: the forward's clamped [x(t - s) | x(t)], and a zero-padded [x(t + s) | x(t)],
        # on the 128x160 / 128x128 tiles as the TDNN-F input gradient builds it (edge row, two-part
        # k-contiguous B)
        Ks = _spliced_k(K)
        add(tile, M, N, Ks, "fwd", a="clamp")
        if tile in ((128, 160), (128, 128)):
            add(tile, M, N, Ks, "bwd", a="p2edge", b="p2")
        else:
            add(tile, M, N, Ks, "bwd", a="zero")
    for epi in ("fwd", "bwd"):
        add((128, 192), 130, 384, 640, epi)   # the boundary of K <= 640
        add((192, 128), 130, 384, 648, epi)   # and the first K past it
        add((128, 160), 130, 320, 72, epi)
    for tile, (M, N, K) in MX_SHAPES.items():
        add(tile, M, N, K, "mx0")
    add((192, 128), *MX_SHAPES[(192, 128)], "mx1")
    # masked A (kf_ops.h: plain or two-part splice with an edge row, k-contiguous B of the same kind)
    for tile, (M, N) in (((384, 160), (400, 160)), ((256, 64), (300, 40)), ((128, 128), (200, 104))):
        add(tile, M, N, 72, "bwd", a="plain", b="kc", masked=True)
        add(tile, M, N, 80, "bwd", a="maskedge", b="p2", masked=True)
    # the edge-row sum over rows inside the ragged last row tile
    add((192, 128), 200, 264, 328, "bwd", edge=(196, 200, 1))
    add((128, 160), 130, 160, 72, "bwd", edge=(128, 130, 0))
    return out


def _seed(c):
    return [c["M"], c["N"], c["K"], sum(map(ord, c["a"] + c["b"])), int(c["masked"])]


@functools.lru_cache(maxsize=2)
def _operands(M, N, K, a, b, masked):
    """the case's operands and their float64 product: unit-normal A, B ~ N(0, 1/K)"""
    rng = np.random.default_rng(_seed(dict(M=M, N=N, K=K, a=a, b=b, masked=masked)))
    rows = np.arange(M)
    W = K if a == "plain" else K // 2
    x = h16(rng.standard_normal((M + 2, W), dtype=np.float32))   # 2 spare rows: an edge row at M
    amask = rng.integers(0, 256, M * W // 8, dtype=np.uint8) if masked else None
    xm = x.astype(np.float64)
    if masked:   # rows >= mask_rows = M (the edge row) are not masked
        xm[:M] *= unpack_bits(amask, M, W)
    if a == "plain":
        A, spec = xm[:M], dict(nparts=1)
    else:
        dts, pol, edges = {"clamp": ((-S, 0), KF_CLAMP, ()), "zero": ((S, 0), KF_ZERO, ()),
                           "p2edge": ((S, 0), KF_ZERO, ((0, 0, M),)),
                           "maskedge": ((0, -S), KF_ZERO, ((1, M - 1, M),))}[a]
        A = splice(xm, rows, dts, pol, edges)
        spec = dict(nparts=2, dt=dts, tpolicy=pol, edges=edges)
    Bm = h16(rng.standard_normal((K, N), dtype=np.float32) / np.sqrt(K))
    B64 = Bm.astype(np.float64)
    acc = A @ B64
    mag = np.abs(A) @ np.abs(B64)
    for arr in (x, Bm, acc, mag):
        arr.setflags(write=False)
    return dict(x=x, W=W, amask=amask, spec=spec, B=Bm, acc=acc, mag=mag)


def fused_inputs(c):
    """everything a fused case reads: operands (shared between the cases of one shape), the
    epilogue's tensors and leading dimensions, and the float64 reference (epilogue_ref)"""
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    ops = _operands(M, N, K, c["a"], c["b"], c["masked"])
    rng = np.random.default_rng(_seed(c) + [sum(map(ord, epi))])
    ldo, ldr, ldo2, ldo8 = N + 8, N + 16, N + 24, N + 32
    d = dict(ops=ops, ldo=ldo, ldr=ldr, ldo2=ldo2, ldo8=ldo8, alpha=1.0, beta=0.0, resid_alpha=0.0,
             relu=False, has_out=epi != "out2only", has_out2=epi in ("bwd", "out2only", "mx1"),
             has_out8=epi in ("mx0", "mx1"), out8_src=int(epi == "mx1"))
    kw = {}
    if epi == "scaled":
        d["alpha"] = 0.5
    if epi in ("fwd", "accum"):
        d["bias"] = kw["bias"] = h16(rng.uniform(-0.5, 0.5, N))
    if epi == "fwd":
        d["relu"] = True
        d["scale"] = kw["scale"] = rng.uniform(0.5, 1.5, N).astype(np.float32)
        d["shift"] = kw["shift"] = (rng.standard_normal(N) * 0.1).astype(np.float32)
    if epi in ("mx0", "mx1"):
        d["relu"] = True
    if epi in ("fwd", "bwd", "out2only"):
        d["resid"] = h16(rng.standard_normal((M, N), dtype=np.float32))
        d["resid_alpha"] = 0.66
        kw["resid"] = d["resid"]
    if d["has_out2"]:
        d["scale2"] = kw["scale2"] = rng.uniform(0.5, 1.5, N).astype(np.float32)
        # random bits in the pad columns too: an index built with the wrong leading dimension reads them
        d["mask_in"] = rng.integers(0, 256, (M + 2) * ldo2 // 8 + 4, dtype=np.uint8)
        kw["mask_in"] = unpack_bits(d["mask_in"], M, ldo2)[:, :N]
    if epi == "accum":
        d["alpha"], d["beta"] = -0.5, 0.75
        d["old"] = kw["old"] = h16(rng.standard_normal((M, N), dtype=np.float32))
    d["ref"] = epilogue_ref(ops["acc"], ops["mag"], K, alpha=d["alpha"], beta=d["beta"], relu=d["relu"],
                            resid_alpha=d["resid_alpha"], **kw)
    return d


def relu_exempt_share(ref, rows=None):
    """share of elements whose ReLU bit the bound leaves open"""
    sure = ref["sure"] if rows is None else ref["sure"][rows]
    return 1.0 - float(np.mean(sure))


# ---------------------------------------------------------------- weight-gradient cases
WGRAD_T = 1000
# tile -> (M, N) of kf_gemm_wgrad's dispatch (dW is [M x N], the reduction runs over T rows);
# M and N are multiples of 8 (operand columns are 16-byte granular) and of no tile dimension
WGRAD_TILES = {
    (320, 256): (600, 264),
    (192, 256): (184, 264),
    (256, 256): (248, 264),
    (192, 128): (184, 104),
    (256, 128): (248, 104),
    (192, 64): (184, 40),
    (256, 64): (248, 40),
    (384, 160): (328, 160),
}


def wgrad_cases():
    """dicts: id, tile, M, N, T, a ('plain' | 'clamp' | 'zero' | 'im2col'), part (two-part A's part
    width), maskb"""
    out = []

    def add(tile, M, N, T=WGRAD_T, a="plain", part=0, maskb=False):
        cid = "%dx%d-%dx%d-T%d-%s%s" % (tile[0], tile[1], M, N, T, a, "-maskedB" if maskb else "")
        out.append(dict(id=cid, tile=tile, M=M, N=N, T=T, a=a, part=part, maskb=maskb))

    for tile, (M, N) in WGRAD_TILES.items():
        add(tile, M, N)
    add((256, 128), 248, 104, T=200)   # at most one split (fewer than 4 K-steps per further split)
    add((256, 128), 248, 104, T=72)
    # the TDNN-F linear's [x(t - s) | x(t)] with parts of one tile's rows: the parts' tiles are
    # paired per XCD (WgradArgs::pair_ps)
    add((384, 160), 768, 160, a="clamp", part=384)
    add((384, 160), 768, 160, a="zero", part=384)
    # the general (im2col) operand on a conv the halo kernel declines (32 input filters):
    # test_gpu_kernels.py's hin 10, fin 32, hout 10, fout 64 at T = 37 frames
    add((192, 64), 288, 64, T=370, a="im2col")
    # masked B (N > 128), A plain and two-part, on the 192-, 256- and 320-row tiles
    for tile, M in (((192, 256), 184), ((256, 256), 248), ((320, 256), 600)):
        add(tile, M, 264, maskb=True)
    for tile, part in (((192, 256), 88), ((256, 256), 128), ((320, 256), 304)):
        add(tile, 2 * part, 264, a="clamp", part=part, maskb=True)
    return out


IM2COL = dict(frames=37, hin=10, fin=32, hout=10, sub=1, offs=[(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)])


def _im2col(x, frames, hin, fin, hout, sub, offs):
    xr = x.reshape(frames, hin, fin)
    t, h = np.repeat(np.arange(frames), hout), np.tile(np.arange(hout), frames)
    parts = []
    for dt, dh in offs:
        ts, hs = t + dt, h * sub + dh
        ok = (ts >= 0) & (ts < frames) & (hs >= 0) & (hs < hin)
        parts.append(np.where(ok[:, None], xr[np.clip(ts, 0, frames - 1), np.clip(hs, 0, hin - 1)], 0.0))
    return np.concatenate(parts, 1)


@functools.lru_cache(maxsize=4)
def _wgrad_inputs(M, N, T, a, part, maskb):
    rng = np.random.default_rng([M, N, T, part, sum(map(ord, a)), int(maskb)])
    if a == "plain":
        x = h16(rng.standard_normal((T, M), dtype=np.float32))
        A = x.astype(np.float64)
    elif a == "im2col":
        g = IM2COL
        x = h16(rng.standard_normal((g["frames"], g["hin"] * g["fin"]), dtype=np.float32))
        A = _im2col(x.astype(np.float64), **g)
    else:
        x = h16(rng.standard_normal((T + 2, part), dtype=np.float32))
        A = splice(x, np.arange(T), (-S, 0), KF_CLAMP if a == "clamp" else KF_ZERO)
    assert A.shape == (T, M)
    Bs = h16(rng.standard_normal((T, N), dtype=np.float32))
    bmask = rng.integers(0, 256, T * N // 8, dtype=np.uint8) if maskb else None
    B = Bs.astype(np.float64)
    if maskb:
        B = B * unpack_bits(bmask, T, N)
    d = dict(x=x, Bs=Bs, bmask=bmask, acc=A.T @ B, mag=np.abs(A).T @ np.abs(B), bsum=B.sum(0),
             bmag=np.abs(B).sum(0),
             col_scale=rng.uniform(0.5, 1.5, N).astype(np.float32) * rng.choice([-1.0, 1.0], N).astype(np.float32),
             old_w=rng.standard_normal((M, N), dtype=np.float32), old_b=rng.standard_normal(N, dtype=np.float32))
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def wgrad_inputs(c):
    return _wgrad_inputs(c["M"], c["N"], c["T"], c["a"], c["part"], c["maskb"])
