"""KfEpilogue.drop (include/kf_ops.h): the per-row-segment column factor of the
fused GEMM epilogue, at kernel level. Row segments start at [0, 5, 37, 128, 129, 384]: one is
shorter than a 32-row epilogue chunk, two boundaries sit at and next to a 128-row tile edge, and
the last row tile is ragged (M = 517, 700). (a) / (b) are element-exact: a factor from
{0.5, 1, 2} commutes with the fp16 rounding, so the launch with drop must equal the plain
launch times the factor, bit for bit, which pins row_seg on every tile. (c) general fp32 factors
against tests/gemm_ref.py's rule extended in tests/dropout_ref.py. (d) the rejected
combinations. (e) kf_dropout_masks / kf_row_seg against the numpy reference."""
import ctypes as C

import numpy as np
import pytest

import dropout_ref as dr
import gemm_ref as gr

pytestmark = pytest.mark.gpu

SHAPES = [(517, 256, 128), (700, 1536, 320)]


def _segs(M):
    return [0, 5, 37, 128, 129, 384, M]


def _up_i32(kf, a):
    a = np.ascontiguousarray(a, np.int32)
    buf = kf.DeviceBuffer(max(a.nbytes, 16))
    kf.check(kf.core.bridge_transfer_int32(buf.ptr, a.ctypes.data, a.size), "upload int32")
    return buf


def _up_u8(kf, a):
    a = np.ascontiguousarray(a, np.uint8)
    pad = np.zeros((a.size + 3) // 4 * 4, np.uint8)
    pad[:a.size] = a.reshape(-1)
    return _up_i32(kf, pad.view(np.int32))


class Problem:
    """operands of one product in the form `variant` names, and what the epilogue reads"""

    def __init__(self, kf, M, N, K, variant, seed):
        rng = np.random.default_rng(seed)
        self.kf, self.M, self.N, self.K = kf, M, N, K
        self.keep = []
        W = K // 2
        w = gr.h16(rng.standard_normal((K, N)) / np.sqrt(K))       # logical B [K x N]
        if variant in ("kc", "rm"):
            a = gr.h16(rng.standard_normal((M, K)) * 0.5)
            self.A64 = a.astype(np.float64)
            da = kf.upload_fp16(a)
            self.a = kf.operand(da.ptr, K, M, K, 1)
        else:   # two-part time splice [x(t - 3) | x(t)], clamped (the TDNN-F forward's form)
            x = gr.h16(rng.standard_normal((M, W)) * 0.5)
            self.A64 = gr.splice(x, np.arange(M), (-3, 0))
            da = kf.upload_fp16(x)
            self.a = kf.operand(da.ptr, W, M, K, 1, nparts=2, part_width=W, tpolicy=gr.KF_CLAMP, dt=(-3, 0))
        self.keep.append(da)
        if variant == "rm":
            db = kf.upload_fp16(w)
            self.b = kf.operand(db.ptr, N, K, N, 0)
        elif variant == "p2p2":   # B[n][p W + kk] = w2[n + p N][kk] (the input gradient's weight rows)
            db = kf.upload_fp16(np.concatenate([w[:W].T, w[W:].T], 0))
            self.b = kf.operand(db.ptr, W, N, K, 1, nparts=2, part_width=W, T=2 * N, dt=(0, N))
        else:
            db = kf.upload_fp16(w.T.copy())
            self.b = kf.operand(db.ptr, K, N, K, 1)
        self.keep.append(db)
        self.B64 = w.astype(np.float64)
        self.rng = rng
        segs = _segs(M)
        self.row_seg = dr.row_segments(segs, M)
        self.nseg = len(segs) - 1
        self.d_row_seg = _up_i32(kf, self.row_seg)

    def table(self, values):
        d = self.kf.upload_f32(np.ascontiguousarray(values, np.float32))
        self.keep.append(d)
        return d

    def run(self, e):
        kf = self.kf
        kf.check(kf.core.kf_gemm_fused(self.M, self.N, self.K, C.byref(self.a), C.byref(self.b), C.byref(e)), "gemm")
        kf.sync()


def _bits16(kf, buf, rows, N):
    return kf.read_fp16(buf.ptr, (rows, N)).view(np.uint16)


def _clear_of_fp16_edges(x16):
    """every nonzero value a normal fp16 with a binade to spare on both sides: times 0.5 or 2
    stays normal and finite, so the power-of-two factor commutes with the rounding"""
    v = np.abs(x16.view(np.float16).astype(np.float64))
    nz = v[v != 0]
    return nz.size > 0 and nz.min() >= 2.0 ** -13 and nz.max() <= 2.0 ** 14


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("variant", ["kc", "p2", "rm"])
def test_forward_power_of_two_factors_exact(gpu, M, N, K, variant):
    """(a) ReLU, scale / shift, no residual: out(drop) == out(plain) * drop[row_seg[m]][n]"""
    kf = gpu
    P = Problem(kf, M, N, K, variant, seed=M + N + len(variant))
    rng = P.rng
    tab = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=(P.nseg, N))
    scale = rng.uniform(0.5, 1.5, N).astype(np.float32)
    shift = rng.uniform(0.25, 1.0, N).astype(np.float32)     # v = relu * scale + shift >= 0.25: no tiny values
    bias = gr.h16(rng.uniform(-0.1, 0.1, N))
    dsc, dsh, dbias, dtab = kf.upload_f32(scale), kf.upload_f32(shift), kf.upload_fp16(bias), P.table(tab)
    outs, masks = [], []
    for with_drop in (False, True):
        out, mask = kf.DeviceBuffer(M * N * 2), kf.DeviceBuffer(M * N // 8 + 16)
        e = kf.KfEpilogue(out=out.ptr, ldo=N, alpha=1.0, bias=dbias.ptr, relu=1, mask_out=mask.ptr, scale=dsc.ptr,
                          shift=dsh.ptr)
        if with_drop:
            e.drop, e.ld_drop, e.row_seg = dtab.ptr, N, P.d_row_seg.ptr
        P.run(e)
        outs.append(_bits16(kf, out, M, N))
        masks.append(kf.read_fp16(mask.ptr, (M * N // 16,)).view(np.uint16))
    plain, dropped = outs
    assert _clear_of_fp16_edges(plain), "the test's magnitudes reach fp16 overflow or subnormals"
    want = (plain.view(np.float16).astype(np.float32) * tab[P.row_seg]).astype(np.float16).view(np.uint16)
    bad = np.argwhere(dropped != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    assert np.array_equal(masks[0], masks[1]), "the ReLU mask changed"
    assert (tab[P.row_seg] != 1).mean() > 0.5   # the factor did something


@pytest.mark.parametrize("M,N,K,edge", [(517, 256, 128, (513, 517)), (700, 1536, 320, (126, 130))])
@pytest.mark.parametrize("variant", ["kc", "p2p2"])
def test_out2_power_of_two_factors_exact(gpu, M, N, K, edge, variant):
    """(b) the input gradient's form: out (g, with the bypass) is untouched, out2 =
    rne(v scale2 drop bit) equals the plain launch's out2 times the factor, and the edge row
    (edge_src = 1: rows at the end of the last tile / across a tile and two segment boundaries)
    is kf_rows_sum of the stored out2"""
    kf = gpu
    P = Problem(kf, M, N, K, variant, seed=M + N + 7)
    rng = P.rng
    tab = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=(P.nseg, N))
    scale2 = rng.uniform(0.5, 1.5, N).astype(np.float32)
    # |acc| stays below 4 (std 0.5), so v = acc + resid keeps |v| >= 1: no tiny out2 values
    resid = gr.h16(rng.choice([-1.0, 1.0], (M, N)) * rng.uniform(5.0, 8.0, (M, N)))
    mk = rng.integers(0, 256, M * N // 8, dtype=np.uint8)
    ds2, dres, dmk, dtab = kf.upload_f32(scale2), kf.upload_fp16(resid), _up_u8(kf, mk), P.table(tab)
    res = []
    for with_drop in (False, True):
        out, out2 = kf.DeviceBuffer(M * N * 2), kf.DeviceBuffer((M + 2) * N * 2)
        ref_edge = kf.DeviceBuffer(N * 2)
        e = kf.KfEpilogue(out=out.ptr, ldo=N, alpha=1.0, resid=dres.ptr, ldr=N, resid_alpha=1.0, out2=out2.ptr, ldo2=N,
                          scale2=ds2.ptr, mask_in=dmk.ptr, edge_out=out2.ptr + M * N * 2, edge_r0=edge[0],
                          edge_r1=edge[1], edge_src=1)
        if with_drop:
            e.drop, e.ld_drop, e.row_seg = dtab.ptr, N, P.d_row_seg.ptr
        P.run(e)
        kf.check(kf.core.kf_rows_sum(ref_edge.ptr, out2.ptr, N, edge[0], edge[1], N), "rows_sum")
        kf.sync()
        res.append((_bits16(kf, out, M, N), _bits16(kf, out2, M + 1, N), _bits16(kf, ref_edge, 1, N)))
    (g0, z0, _), (g1, z1, e1) = res
    assert np.array_equal(g0, g1), "out (the unmasked gradient) changed"
    assert _clear_of_fp16_edges(z0[:M]), "the test's magnitudes reach fp16 overflow or subnormals"
    bits = gr.unpack_bits(mk, M, N)
    assert np.all((z0[:M] & 0x7FFF != 0) == bits), "mask_in of the plain launch"
    want = (z0[:M].view(np.float16).astype(np.float32) * tab[P.row_seg]).astype(np.float16).view(np.uint16)
    bad = np.argwhere(z1[:M] != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    assert np.array_equal(z1[M], e1[0]), "edge row differs from kf_rows_sum of the stored out2"
    assert not np.array_equal(z1[M], z0[M])


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_general_factors_against_reference(gpu, M, N, K):
    """(c) fp32 factors in [0, 2]: the forward (bias, ReLU, scale / shift, bypass) and the input
    gradient (out + out2 with scale2, mask_in, bypass), within gemm_ref's tolerance"""
    kf = gpu
    P = Problem(kf, M, N, K, "p2", seed=M + 11)
    rng = P.rng
    acc, mag = P.A64 @ P.B64, np.abs(P.A64) @ np.abs(P.B64)
    tab = rng.uniform(0.0, 2.0, (P.nseg, N)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, N).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, N).astype(np.float32)
    bias = gr.h16(rng.uniform(-0.1, 0.1, N))
    resid = gr.h16(rng.standard_normal((M, N)))
    alpha_r = 0.66
    dsc, dsh, dbias, dres, dtab = (kf.upload_f32(scale), kf.upload_f32(shift), kf.upload_fp16(bias), kf.upload_fp16(resid),
                                   P.table(tab))
    # forward
    out, mask = kf.DeviceBuffer(M * N * 2), kf.DeviceBuffer(M * N // 8 + 16)
    e = kf.KfEpilogue(out=out.ptr, ldo=N, alpha=1.0, bias=dbias.ptr, relu=1, mask_out=mask.ptr, scale=dsc.ptr, shift=dsh.ptr,
                      resid=dres.ptr, ldr=N, resid_alpha=alpha_r, drop=dtab.ptr, ld_drop=N, row_seg=P.d_row_seg.ptr)
    P.run(e)
    ref = dr.epilogue_drop_ref(acc, mag, K, tab, P.row_seg, scale=scale, shift=shift, bias=bias, relu=True, resid=resid,
                               resid_alpha=alpha_r)
    got = kf.read_fp16(out.ptr, (M, N)).astype(np.float64)
    # (ReLU is 1-Lipschitz: the bound at the pre-activation covers either decision of an uncertain bit)
    err = np.abs(got - ref["v"])
    print("forward: max err / tol = %.3f" % float(np.max(err / ref["tol"])))
    assert np.all(err <= ref["tol"]), float(np.max(err - ref["tol"]))
    bits = gr.unpack_bits(kf.read_fp16(mask.ptr, (M * N // 16,)).view(np.uint8), M, N)
    assert np.array_equal(bits[ref["sure"]], ref["bits"][ref["sure"]]), "ReLU mask bits"
    # input gradient
    scale2 = rng.uniform(0.5, 1.5, N).astype(np.float32)
    mk = rng.integers(0, 256, M * N // 8, dtype=np.uint8)
    ds2, dmk = kf.upload_f32(scale2), _up_u8(kf, mk)
    g, dz = kf.DeviceBuffer(M * N * 2), kf.DeviceBuffer(M * N * 2)
    e = kf.KfEpilogue(out=g.ptr, ldo=N, alpha=1.0, resid=dres.ptr, ldr=N, resid_alpha=alpha_r, out2=dz.ptr, ldo2=N,
                      scale2=ds2.ptr, mask_in=dmk.ptr, drop=dtab.ptr, ld_drop=N, row_seg=P.d_row_seg.ptr)
    P.run(e)
    ref = dr.epilogue_drop_ref(acc, mag, K, tab, P.row_seg, scale2=scale2, mask_in=gr.unpack_bits(mk, M, N), resid=resid,
                               resid_alpha=alpha_r)
    got_g = kf.read_fp16(g.ptr, (M, N)).astype(np.float64)
    got_z = kf.read_fp16(dz.ptr, (M, N)).astype(np.float64)
    print("dgrad: max err / tol = %.3f (out), %.3f (out2)" % (float(np.max(np.abs(got_g - ref["v"]) / ref["tol"])),
                                                              float(np.max(np.abs(got_z - ref["out2"]) / ref["tol2"]))))
    assert np.all(np.abs(got_g - ref["v"]) <= ref["tol"])
    assert np.all(np.abs(got_z - ref["out2"]) <= ref["tol2"])


def test_rejected_combinations(gpu):
    """(d) drop with neither or both of scale / out2, without row_seg, with row_group, out8, an
    MXFP8 or a masked operand, a misaligned or too narrow table, or on a tile without the variant"""
    kf = gpu
    M, N, K = 256, 256, 128
    P = Problem(kf, M, N, K, "kc", seed=3)
    tab = P.table(np.ones((P.nseg, N + 8), np.float32))
    ones = kf.upload_f32(np.ones(N, np.float32))
    out, out2 = kf.DeviceBuffer(M * N * 2), kf.DeviceBuffer(M * N * 2)
    q8, s8 = kf.DeviceBuffer(M * N), kf.DeviceBuffer(M * N // 32)
    mk = _up_u8(kf, np.full(M * K // 8, 255, np.uint8))

    def epi(**kw):
        base = dict(out=out.ptr, ldo=N, alpha=1.0, drop=tab.ptr, ld_drop=N + 8, row_seg=P.d_row_seg.ptr)
        base.update(kw)
        return kf.KfEpilogue(**base)

    fwd = dict(scale=ones.ptr, shift=ones.ptr)

    def rejected(e, a=None, b=None, shape=(M, N, K), match="drop"):
        kf.core.kf_clear_error()
        rc = kf.core.kf_gemm_fused(*shape, C.byref(a or P.a), C.byref(b or P.b), C.byref(e))
        msg = (kf.core.kf_last_error() or b"").decode()
        assert rc != 0 and match in msg, (rc, msg)

    rejected(epi())                                                          # neither scale nor out2
    rejected(epi(out2=out2.ptr, ldo2=N, **fwd))                              # both
    rejected(epi(row_seg=None, **fwd))                                       # no row_seg
    rejected(epi(row_group=4, row_stride=8, **fwd))                          # grouped rows
    rejected(epi(out8=q8.ptr, ldo8=N, scale8=s8.ptr, **fwd))                 # MXFP8 copy
    rejected(epi(drop=tab.ptr + 4, **fwd))                                   # misaligned table
    rejected(epi(ld_drop=N - 8, **fwd))                                      # narrower than N
    rejected(epi(ld_drop=N + 4, **fwd))                                      # ld_drop % 8
    # a masked A operand
    am = kf.operand(P.keep[0].ptr, K, M, K, 1, mask=mk.ptr, mask_rows=M)
    rejected(epi(out=None, out2=out2.ptr, ldo2=N), a=am)
    # MXFP8 operands (e4m3 bytes + E8M0 scales)
    a8, b8 = kf.DeviceBuffer(M * K), kf.DeviceBuffer(N * K)
    sa, sb = kf.DeviceBuffer(M * K // 32), kf.DeviceBuffer(N * K // 32)
    for buf, n in ((a8, M * K), (b8, N * K), (sa, M * K // 32), (sb, N * K // 32)):
        kf.core.bridge_gpu_memset(buf.ptr, 0, n)
    ax = kf.operand(a8.ptr, K, M, K, 1, scales=sa.ptr, lds=K // 32)
    bx = kf.operand(b8.ptr, K, N, K, 1, scales=sb.ptr, lds=K // 32)
    rejected(epi(**fwd), a=ax, b=bx)
    # tiles without the variant: N = 160 (384x160 / 128x160) and N = 64 (256x64)
    for n in (160, 64):
        wb = kf.upload_fp16(np.zeros((n, K), np.float16))
        rejected(epi(ldo=n, **fwd), b=kf.operand(wb.ptr, K, n, K, 1), shape=(M, n, K))
    kf.core.kf_clear_error()


def test_masks_match_reference_and_repeat(gpu):
    """(e) kf_dropout_masks against the numpy rule within 1 fp32 ulp (numpy rounds the multiply
    and the add separately), identical for the same (seed, step), different for another step;
    p = 0 entries are skipped"""
    kf = gpu
    B, seed = 5, 0xFEDCBA9876543210
    dims, ps, ords = [256, 1536, 64], [0.3, 0.5, 0.0], [0, 3, 7]
    bufs = [kf.DeviceBuffer(B * d * 4) for d in dims]
    for b, d in zip(bufs, dims):
        kf.core.bridge_gpu_memset(b.ptr, 0, B * d * 4)
    tab = (kf.KfDropLayer * 3)(*[kf.KfDropLayer(mask=b.ptr, ld=d, dim=d, ordinal=o, p=p) for b, d, p, o in
                                 zip(bufs, dims, ps, ords)])

    def draw(step):
        kf.check(kf.core.kf_dropout_masks(3, C.addressof(tab), B, seed, step), "kf_dropout_masks")
        kf.sync()
        return [kf.read_f32(b.ptr, (B, d)) for b, d in zip(bufs, dims)]

    m1, m2, m3 = draw(11), draw(11), draw(12)
    for i in range(2):
        ref = dr.dropout_masks(seed, 11, ords[i], B, dims[i], ps[i])
        ulp = np.spacing(np.maximum(np.abs(ref), np.abs(m1[i])))
        assert np.all(np.abs(m1[i].astype(np.float64) - ref) <= ulp), (i, float(np.max(np.abs(m1[i] - ref) / ulp)))
        assert np.array_equal(m1[i], m2[i]) and not np.array_equal(m1[i], m3[i])
        assert m1[i].min() >= 1 - 2 * ps[i] - 1e-6 and m1[i].max() <= 1 + 2 * ps[i] + 1e-6
    assert not m1[2].any(), "a p = 0 entry was written"
    # bad arguments launch nothing
    bad = (kf.KfDropLayer * 1)(kf.KfDropLayer(mask=bufs[0].ptr, ld=256, dim=256, ordinal=0, p=0.6))
    assert kf.core.kf_dropout_masks(1, C.addressof(bad), B, seed, 0) != 0
    assert kf.core.kf_dropout_masks(3, C.addressof(tab), B, seed, -1) != 0
    kf.core.kf_clear_error()


@pytest.mark.parametrize("T,tc0,tc", [(700, 0, 0), (700, 234, 236), (50, 17, 19)])
def test_row_seg_matches_reference(gpu, T, tc0, tc):
    kf = gpu
    so = np.array([0, 5, 37, T - 3, T], np.int32)
    dso, out = _up_i32(kf, so), kf.DeviceBuffer(T * 4)
    kf.check(kf.core.kf_row_seg(out.ptr, dso.ptr, len(so) - 1, T, tc0, tc), "kf_row_seg")
    kf.sync()
    rows = tc if tc else T
    got = kf.read_f32(out.ptr, (rows,)).view(np.int32)
    assert np.array_equal(got, dr.row_segments(so, T, tc0, tc))
    # one sequence: all zeros
    kf.check(kf.core.kf_row_seg(out.ptr, None, 0, T, tc0, tc), "kf_row_seg")
    kf.sync()
    assert not kf.read_f32(out.ptr, (rows,)).view(np.int32).any()
