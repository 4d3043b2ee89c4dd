"""Direct tests of the public entry points of csrc/ivector.hip (include/kf_ops.h) against
the plain fp64 references of tests/layer_ref.py, at the geometries the network configs never
reach. Integer-valued inputs must come back bit-identical, Gaussian inputs within the fp32
accumulation bound plus one fp16 ulp, copies bit-exact; every output sits in a poisoned buffer
wider than its logical width (see test_gpu_layer_kernels.py)."""
import numpy as np
import pytest

import layer_ref as R
from layer_dev import (NAN16, POISON32, check_padding, gauss, iarr, ints, padded, poison16, rd_u16, rd_u32,
                       rejected, same_bits16, up_u16, up_u32, within)

pytestmark = pytest.mark.gpu


def _data(kind, rng, shape, lim=3):
    return ints(rng, shape, -lim, lim) if kind == "int" else gauss(rng, shape)


# ---------------------------------------------------------------- combine-feature-maps
@pytest.mark.parametrize("T,height,nf1,nf2,seq_off", [
    (1, 1, 1, 1, [0, 0, 1]),
    (50, 7, 3, 2, [0, 10, 10, 37, 50]),
    (301, 40, 1, 5, [0, 1, 16, 32, 49, 49, 301]),
])
def test_combine_feature_maps(gpu, T, height, nf1, nf2, seq_off):
    kf = gpu
    rng = np.random.default_rng(T)
    B = len(seq_off) - 1
    wa, wb, wo = height * nf1, height * nf2, height * (nf1 + nf2)
    lda, ldb, ldo = wa + 3, wb + 5, wo + 7
    a, b, bt = gauss(rng, (T, wa)), gauss(rng, (B, wb)), gauss(rng, (T, wb))
    da, db, dbt = up_u16(kf, padded(a, lda)), up_u16(kf, padded(b, ldb)), up_u16(kf, padded(bt, ldb))
    dso = up_u32(kf, np.asarray(seq_off, np.int32))
    for bsrc, bdev, so, sodev in ((b, db, seq_off, dso.ptr), (bt, dbt, None, None)):
        dout = up_u16(kf, poison16(T + 1, ldo))
        kf.check(kf.core.kf_combine_feature_maps(da.ptr, lda, bdev.ptr, ldb, sodev, B, dout.ptr, ldo, T, height,
                                                 nf1, nf2), "combine_feature_maps")
        kf.sync()
        img = rd_u16(kf, dout.ptr, (T + 1, ldo))
        check_padding(img, T, wo, NAN16)
        ref = R.combine_fm(a, bsrc, so, T, height, nf1, nf2)
        assert np.array_equal(img[:T, :wo], ref.view(np.uint16))


_BWD_LENS = [0, 1, 15, 16, 17, 300]      # around the kernel's 16 frame groups, and an empty sequence


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("height,nf1,nf2", [(7, 0, 2), (7, 3, 2), (8, 0, 8), (8, 2, 8), (13, 0, 5), (13, 4, 5),
                                            (40, 1, 5)])
def test_combine_feature_maps_backward(gpu, height, nf1, nf2, kind):
    kf = gpu
    rng = np.random.default_rng(height * 10 + nf1)
    seq_off = np.concatenate([[0], np.cumsum(_BWD_LENS)]).astype(np.int32)
    T, B = int(seq_off[-1]), len(_BWD_LENS)
    nb, wy = height * nf2, height * (nf1 + nf2)
    ldy, ldb = wy + 3, nb + 5
    dy = _data(kind, rng, (T, wy))
    ddy, dso = up_u16(kf, padded(dy, ldy)), up_u32(kf, seq_off)
    runs = []
    for _ in range(2):
        ddb = up_u16(kf, poison16(B + 1, ldb))
        kf.check(kf.core.kf_combine_feature_maps_backward(ddy.ptr, ldy, dso.ptr, B, ddb.ptr, ldb, height, nf1, nf2),
                 "combine_feature_maps_backward")
        kf.sync()
        runs.append(rd_u16(kf, ddb.ptr, (B + 1, ldb)))
    img = runs[0]
    assert np.array_equal(runs[0], runs[1]), "not deterministic"
    check_padding(img, B, nb, NAN16)
    got = img[:B, :nb].view(np.float16)
    ref = R.combine_fm_bwd(dy, seq_off, height, nf1, nf2)
    assert np.all(img[0, :nb] == 0)      # the empty sequence's row is written, as zeros
    if kind == "int":
        same_bits16(got, ref)
    else:
        S = R.combine_fm_bwd(np.abs(R.f64(dy)), seq_off, height, nf1, nf2)
        within(got, ref, R.acc_bound(np.asarray(_BWD_LENS)[:, None], S, ref))


# ---------------------------------------------------------------- small-fin conv as im2col
_TAPSETS = {"3x3": R.taps(R.T3, R.T3), "2tap": R.taps((0, 1), (1,))}


def _small_geoms():
    for fin in (1, 3, 6, 8):
        for tapset in _TAPSETS:
            for sub in (1, 2):
                for T in (1, 23):
                    yield pytest.param(fin, tapset, sub, T, id=f"fin{fin}-{tapset}-sub{sub}-T{T}")


def _kps(ntaps, fin):
    k = (ntaps * fin + 7) // 8 * 8
    return (k, 64 if ntaps * fin == 54 else k + 8)


@pytest.mark.parametrize("fin,tapset,sub,T", list(_small_geoms()))
def test_im2col_small(gpu, fin, tapset, sub, T):
    kf = gpu
    dt, dh = _TAPSETS[tapset]
    hin, hout = 10, 10 // sub
    rng = np.random.default_rng(fin * 100 + T)
    x = gauss(rng, (T, hin * fin))
    ldx = hin * fin + 3
    dx = up_u16(kf, padded(x, ldx))
    for kp in _kps(len(dt), fin):
        dP = up_u16(kf, poison16(T * hout + 1, kp))
        kf.check(kf.core.kf_im2col_small(dx.ptr, ldx, T, hin, hout, sub, fin, len(dt), iarr(dt), iarr(dh), dP.ptr, kp),
                 "im2col_small")
        kf.sync()
        img = rd_u16(kf, dP.ptr, (T * hout + 1, kp))
        check_padding(img, T * hout, kp, NAN16)
        ref = R.im2col_small(x, T, hin, hout, sub, fin, dt, dh, kp)
        assert np.array_equal(img[:T * hout], ref.view(np.uint16)), kp


@pytest.mark.parametrize("kp,ntaps,needle", [
    (12, 9, "kp must be a multiple of 8"),
    (8, 9, "bad shape"),
    (16, 10, "bad shape"),
])
def test_im2col_small_rejects(gpu, kp, ntaps, needle):
    kf = gpu
    T, h = 3, 6
    dx, dP = up_u16(kf, np.zeros((T, h), np.float16)), up_u16(kf, poison16(T * h, 16))
    dt, dh = [0] * ntaps, [0] * ntaps
    rc = kf.core.kf_im2col_small(dx.ptr, h, T, h, h, 1, 1, ntaps, iarr(dt), iarr(dh), dP.ptr, kp)
    rejected(kf, rc, "kf_im2col_small: " + needle, "kf_last_error")
    kf.sync()
    assert np.all(rd_u16(kf, dP.ptr, (T * h, 16)) == NAN16)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("fin,tapset,sub,T", list(_small_geoms()))
def test_col2im_small(gpu, fin, tapset, sub, T, kind):
    kf = gpu
    dt, dh = _TAPSETS[tapset]
    hin, hout = 10, 10 // sub
    rng = np.random.default_rng(fin * 100 + T + 1)
    wd = hin * fin
    ldx = wd + 5
    for kp in _kps(len(dt), fin):
        dP = _data(kind, rng, (T * hout, kp))      # the columns >= ntaps*fin hold data too: never read
        ddP = up_u16(kf, dP)
        ddx = up_u16(kf, poison16(T + 1, ldx))
        kf.check(kf.core.kf_col2im_small(ddP.ptr, T, hin, hout, sub, fin, len(dt), iarr(dt), iarr(dh), kp, ddx.ptr,
                                         ldx), "col2im_small")
        kf.sync()
        img = rd_u16(kf, ddx.ptr, (T + 1, ldx))
        check_padding(img, T, wd, NAN16)
        got = img[:T, :wd].view(np.float16)
        ref = R.col2im_small(dP, T, hin, hout, sub, fin, dt, dh, kp)
        if kind == "int":
            same_bits16(got, ref)
        else:
            S = R.col2im_small(np.abs(R.f64(dP)), T, hin, hout, sub, fin, dt, dh, kp)
            within(got, ref, R.acc_bound(len(dt), S, ref))


# ---------------------------------------------------------------- per-sequence linear component
_ROWS_SHAPES = [(1, 1, 1), (5, 7, 13), (3, 100, 200)]


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("Rr,K,N", _ROWS_SHAPES)
def test_rows_gemm(gpu, Rr, K, N, kind):
    kf = gpu
    rng = np.random.default_rng(K + N)
    x, W = _data(kind, rng, (Rr, K)), _data(kind, rng, (K, N))
    ldx, ldw, ldy = K + 3, N + 5, N + 7
    dx, dw = up_u16(kf, padded(x, ldx)), up_u16(kf, padded(W, ldw))
    dy = up_u16(kf, poison16(Rr + 1, ldy))
    kf.check(kf.core.kf_rows_gemm(dx.ptr, ldx, dw.ptr, ldw, dy.ptr, ldy, Rr, K, N), "rows_gemm")
    kf.sync()
    img = rd_u16(kf, dy.ptr, (Rr + 1, ldy))
    check_padding(img, Rr, N, NAN16)
    got = img[:Rr, :N].view(np.float16)
    ref = R.f64(x) @ R.f64(W)
    if kind == "int":
        same_bits16(got, ref)
    else:
        within(got, ref, R.acc_bound(K, np.abs(R.f64(x)) @ np.abs(R.f64(W)), ref))


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("Rr,M,N", _ROWS_SHAPES)
def test_rows_wgrad(gpu, Rr, M, N, kind):
    kf = gpu
    rng = np.random.default_rng(M + N + 1)
    x, g = _data(kind, rng, (Rr, M)), _data(kind, rng, (Rr, N))
    ldx, ldg, ldd = M + 3, N + 5, N + 7
    dx, dg = up_u16(kf, padded(x, ldx)), up_u16(kf, padded(g, ldg))
    dW = up_u32(kf, np.full((M + 1, ldd), POISON32, np.uint32))
    kf.check(kf.core.kf_rows_wgrad(dx.ptr, ldx, dg.ptr, ldg, dW.ptr, ldd, Rr, M, N), "rows_wgrad")
    kf.sync()
    img = rd_u32(kf, dW.ptr, (M + 1, ldd))
    check_padding(img, M, N, POISON32)
    got = img[:M, :N].view(np.float32)
    ref = R.f64(x).T @ R.f64(g)
    if kind == "int":
        assert np.array_equal(got, ref)
    else:
        within(got, ref, R.acc_bound(Rr, np.abs(R.f64(x)).T @ np.abs(R.f64(g))))


# ---------------------------------------------------------------- kf_scale_cols
def _scale_sets():
    """constant columns of scales with few bits, and per-column random scales whose products
    need more than 24 bits: only there can rne_fp16(rne_fp32(x * s)) differ from one rounding"""
    rng = np.random.default_rng(11)
    for s in (1.0, 0.5, 3.0, 1 + 2.0 ** -12, -(1 - 2.0 ** -13), 1.0 / 3.0):
        yield np.full(2048, s, np.float32)
    for _ in range(12):
        yield (rng.uniform(0.5, 2.0, 2048) * rng.choice([-1.0, 1.0], 2048)).astype(np.float32)


def _scale_ref(x, scale):
    with np.errstate(over="ignore", invalid="ignore"):
        return (x.astype(np.float32) * scale[None, :]).astype(np.float16)


def test_scale_cols_rounds_twice(gpu):
    """y = rne_fp16(rne_fp32(x * scale)) over every fp16 bit pattern (32 x 2048), out of place
    and in place"""
    kf = gpu
    # (shuffled: in counting order a column would hold one mantissa 32 times)
    x = np.random.default_rng(12).permutation(65536).astype(np.uint16).reshape(32, 2048).view(np.float16)
    ld = 2048 + 8
    told_apart = 0
    for k, scale in enumerate(_scale_sets()):
        ref = _scale_ref(x, scale)
        with np.errstate(over="ignore", invalid="ignore"):
            once = (x.astype(np.float64) * scale.astype(np.float64)[None, :]).astype(np.float16)   # exact product
        nan = np.isnan(ref)
        told_apart += int(np.count_nonzero(ref.view(np.uint16)[~nan] != once.view(np.uint16)[~nan]))
        ds = up_u32(kf, scale)
        for inplace in ((False, True) if k % 3 == 0 else (False,)):
            dx = up_u16(kf, padded(x, ld, extra_rows=1))
            dy = dx if inplace else up_u16(kf, poison16(33, ld))
            kf.check(kf.core.kf_scale_cols(dx.ptr, ld, ds.ptr, dy.ptr, ld, 32, 2048), "scale_cols")
            kf.sync()
            img = rd_u16(kf, dy.ptr, (33, ld))
            check_padding(img, 32, 2048, NAN16)
            got = img[:32, :2048]
            assert np.array_equal(np.isnan(got.view(np.float16)), nan)
            bad = np.flatnonzero(got[~nan] != ref.view(np.uint16)[~nan])
            assert bad.size == 0, (k, inplace, bad.size, x[~nan][bad[0]], scale[np.nonzero(~nan)[1][bad[0]]])
    assert told_apart >= 8      # the data does tell one rounding from two
