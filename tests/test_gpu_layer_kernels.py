"""Direct tests of the public entry points of csrc/layers.hip (include/kf_ops.h), and of
kf_rows_sum / kf_rows_sum_mask which other tests use as their reference, against the plain
fp64 references of tests/layer_ref.py.

Two kinds of input. Integer-valued fp16 data keeps every product and partial sum exact in fp32
and every result exact in fp16, so the kernel must be bit-identical to the reference whatever
its summation order: a dropped, duplicated or mis-indexed term cannot hide, and the many exact
zeros pin the ReLU's `> 0`. Gaussian data checks the rounding points, per element within
n_terms * 2^-24 * sum|terms| + 2^-10 |ref| + 2^-24 (fp32 accumulation plus one fp16 ulp; fp32
outputs drop the fp16 term). Outputs live in poisoned buffers wider / longer than the logical
result, and everything outside it must come back unchanged."""
import numpy as np
import pytest

import layer_ref as R
from layer_dev import (NAN16, POISON32, check_padding, gauss, iarr, ints, padded, poison16, poison32, rd_bytes,
                       rd_u16, rd_u32, rejected, same_bits16, up_bytes, up_u16, up_u32, within)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- kf_small_gemm
@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("T,K,N", [(1, 1, 8), (5, 13, 24), (37, 40, 40), (300, 64, 64)])
def test_small_gemm(gpu, T, K, N, kind):
    kf = gpu
    rng = np.random.default_rng(T * 100 + K)
    mk = ints if kind == "int" else gauss
    x = mk(rng, (T, K), -3, 3) if kind == "int" else mk(rng, (T, K))
    M = mk(rng, (K, N), -3, 3) if kind == "int" else mk(rng, (K, N))
    ldx, ldy = K + 3, N + 8
    dx, dm = up_u16(kf, padded(x, ldx)), up_u16(kf, M)
    dy = up_u16(kf, poison16(T + 1, ldy))
    kf.check(kf.core.kf_small_gemm(dx.ptr, ldx, dm.ptr, dy.ptr, ldy, T, K, N), "small_gemm")
    kf.sync()
    img = rd_u16(kf, dy.ptr, (T + 1, ldy))
    check_padding(img, T, N, NAN16)
    got = img[:T, :N].view(np.float16)
    ref = R.f64(x) @ R.f64(M)
    if kind == "int":
        same_bits16(got, ref)
    else:
        within(got, ref, R.acc_bound(K, np.abs(R.f64(x)) @ np.abs(R.f64(M)), ref))


@pytest.mark.parametrize("K,N", [(65, 64), (64, 72), (8, 12)])
def test_small_gemm_rejects(gpu, K, N):
    kf = gpu
    dx, dm = up_u16(kf, np.zeros((4, 80), np.float16)), up_u16(kf, np.zeros((80, 80), np.float16))
    dy = up_u16(kf, poison16(4, 80))
    rejected(kf, kf.core.kf_small_gemm(dx.ptr, 80, dm.ptr, dy.ptr, 80, 4, K, N), f"small_gemm: K={K} N={N}")
    kf.sync()
    assert np.all(rd_u16(kf, dy.ptr, (4, 80)) == NAN16)


# ---------------------------------------------------------------- kf_bn_apply
def _fp16_ulp(v):
    a = np.maximum(np.abs(R.f64(v)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("rows,D", [(1, 1), (13, 37), (7, 1536)])
def test_bn_apply(gpu, rows, D, kind):
    kf = gpu
    rng = np.random.default_rng(rows + D)
    if kind == "int":   # |x| <= 64, scale 2^-2 .. 2^2, shift a multiple of 0.5: exact below 512
        x = ints(rng, (rows, D), -64, 64)
        scale = (2.0 ** rng.integers(-2, 3, D)).astype(np.float32)
        shift = (0.5 * rng.integers(-16, 17, D)).astype(np.float32)
    else:
        x = gauss(rng, (rows, D))
        scale = rng.uniform(0.5, 1.5, D).astype(np.float32) * rng.choice([-1, 1], D).astype(np.float32)
        shift = gauss(rng, D, np.float32)
    dx, ds, dh = up_u16(kf, x), up_u32(kf, scale), up_u32(kf, shift)
    dy = up_u16(kf, poison16(rows + 1, D))
    kf.check(kf.core.kf_bn_apply(dx.ptr, dy.ptr, rows, D, ds.ptr, dh.ptr), "bn_apply")
    kf.sync()
    img = rd_u16(kf, dy.ptr, (rows + 1, D))
    check_padding(img, rows, D, NAN16)
    got = img[:rows].view(np.float16)
    ref = R.f64(x) * R.f64(scale) + R.f64(shift)
    if kind == "int":
        same_bits16(got, ref)
    else:
        within(got, ref, _fp16_ulp(ref))


# ---------------------------------------------------------------- kf_conv_c1_forward / wgrad
def _c1_inputs(geom, kind):
    T, hin, hout, sub, fout, dts, dhs = geom
    dt, dh = R.taps(dts, dhs)
    rng = np.random.default_rng(T * 1000 + fout)
    if kind == "int":   # |pre| <= 9*6 + 4, |y| <= 58*4 + 8: exact in fp16 (multiples of 0.5)
        x, W, b = ints(rng, (T, hin), -3, 3), ints(rng, (len(dt), fout), -2, 2), ints(rng, fout, -4, 4)
        scale = (2.0 ** rng.integers(-1, 3, fout)).astype(np.float32)
        shift = (0.5 * rng.integers(-16, 17, fout)).astype(np.float32)
        dz = ints(rng, (T * hout, fout), -2, 2)
    else:
        x, W, b = gauss(rng, (T, hin)), gauss(rng, (len(dt), fout)), gauss(rng, fout)
        scale = rng.uniform(0.5, 1.5, fout).astype(np.float32)
        shift = gauss(rng, fout, np.float32)
        dz = gauss(rng, (T * hout, fout))
    return dt, dh, x, W, b, scale, shift, dz


@pytest.mark.parametrize("full", [True, False], ids=["epilogue", "null"])
@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("geom", R.C1_GEOMS, ids=lambda g: f"T{g[0]}h{g[1]}-{g[2]}s{g[3]}f{g[4]}t{len(g[5]) * len(g[6])}")
def test_conv_c1_forward(gpu, geom, kind, full):
    kf = gpu
    T, hin, hout, sub, fout = geom[:5]
    dt, dh, x, W, b, scale, shift, _ = _c1_inputs(geom, kind)
    noff, rows = len(dt), T * hout
    n = rows * fout
    dx, dw = up_u16(kf, x), up_u16(kf, W)
    db, ds, dsh = up_u16(kf, b), up_u32(kf, scale), up_u32(kf, shift)
    dy = up_u16(kf, poison16(rows + 2, fout))
    dm = up_bytes(kf, np.full(n // 8 + 8, 0xA5, np.uint8))
    kf.check(kf.core.kf_conv_c1_forward(T, hin, hout, sub, fout, noff, iarr(dt), iarr(dh), dx.ptr, dw.ptr,
                                        db.ptr if full else None, ds.ptr if full else None,
                                        dsh.ptr if full else None, dy.ptr, dm.ptr if full else None),
             "conv_c1_forward")
    kf.sync()
    img = rd_u16(kf, dy.ptr, (rows + 2, fout))
    check_padding(img, rows, fout, NAN16)
    got = img[:rows].view(np.float16)
    mbytes = rd_bytes(kf, dm.ptr, n // 8 + 8)
    assert np.all(mbytes[n // 8:] == 0xA5)
    if not full:
        assert np.all(mbytes == 0xA5)
    b_, sc_, sh_ = (b, scale, shift) if full else (None, None, None)
    pre, mask, ref = R.conv_c1(x, W, b_, sc_, sh_, T, hin, hout, sub, dt, dh)
    gmask = R.unpack_bits(mbytes, n).reshape(rows, fout)
    if kind == "int":
        same_bits16(got, ref)
        if full:
            assert np.array_equal(gmask, mask)
        return
    # terms of y: the noff products and the bias, each times scale, and the shift (noff + 2);
    # terms of the pre-activation: the products and the bias (noff + 1)
    absb = np.abs(R.f64(b)) if full else None
    S_pre = R.conv_c1(np.abs(R.f64(x)), np.abs(R.f64(W)), absb, None, None, T, hin, hout, sub, dt, dh)[0]
    S = S_pre * np.abs(R.f64(scale)) + np.abs(R.f64(shift)) if full else S_pre
    within(got, ref, R.acc_bound(noff + 2, S, ref))
    if full:
        decided = np.abs(pre) > (noff + 1) * R.F32_U * S_pre
        assert np.array_equal(gmask[decided], mask[decided])
        assert 1.0 - decided.mean() <= 1e-3


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("geom", R.C1_GEOMS, ids=lambda g: f"T{g[0]}h{g[1]}-{g[2]}s{g[3]}f{g[4]}t{len(g[5]) * len(g[6])}")
def test_conv_c1_wgrad(gpu, geom, kind, with_db):
    kf = gpu
    T, hin, hout, sub, fout = geom[:5]
    dt, dh, x, _, _, _, _, dz = _c1_inputs(geom, kind)
    noff = len(dt)
    dx, dzb = up_u16(kf, x), up_u16(kf, dz)
    dW, db = up_u32(kf, poison32(noff * fout + 16)), up_u32(kf, poison32(fout + 16))
    kf.check(kf.core.kf_conv_c1_wgrad(T, hin, hout, sub, fout, noff, iarr(dt), iarr(dh), dx.ptr, dzb.ptr, dW.ptr,
                                      db.ptr if with_db else None), "conv_c1_wgrad")
    kf.sync()
    gW, gb = rd_u32(kf, dW.ptr, (noff * fout + 16,)), rd_u32(kf, db.ptr, (fout + 16,))
    assert np.all(gW[noff * fout:] == POISON32) and np.all(gb[fout if with_db else 0:] == POISON32)
    rW, rb = R.conv_c1_wgrad(x, dz, T, hin, hout, sub, dt, dh)
    gW = gW[:noff * fout].view(np.float32).reshape(noff, fout)
    gb = gb[:fout].view(np.float32)
    if kind == "int":
        assert np.array_equal(gW, rW) and (not with_db or np.array_equal(gb, rb))
        return
    SW, Sb = R.conv_c1_wgrad(np.abs(R.f64(x)), np.abs(R.f64(dz)), T, hin, hout, sub, dt, dh)
    within(gW, rW, R.acc_bound(T * hout, SW))
    if with_db:
        within(gb, rb, R.acc_bound(T * hout, Sb))


def test_conv_c1_wgrad_no_frames(gpu):
    """T = 0: empty sums, no launch"""
    kf = gpu
    dt, dh = R.taps(R.T3, R.T3)
    dx, dz = up_u16(kf, np.zeros(64, np.float16)), up_u16(kf, np.zeros(64, np.float16))
    dW, db = up_u32(kf, poison32(9 * 32 + 16)), up_u32(kf, poison32(32 + 16))
    assert kf.core.kf_conv_c1_wgrad(0, 40, 40, 1, 32, 9, iarr(dt), iarr(dh), dx.ptr, dz.ptr, dW.ptr, db.ptr) == 0
    kf.sync()
    gW, gb = rd_u32(kf, dW.ptr, (9 * 32 + 16,)), rd_u32(kf, db.ptr, (32 + 16,))
    assert np.all(gW[:9 * 32] == 0) and np.all(gb[:32] == 0)
    assert np.all(gW[9 * 32:] == POISON32) and np.all(gb[32:] == POISON32)
    assert kf.core.kf_conv_c1_wgrad(0, 40, 40, 1, 32, 9, iarr(dt), iarr(dh), dx.ptr, dz.ptr, dW.ptr, None) == 0
    kf.sync()


@pytest.mark.parametrize("fout,noff", [(24, 9), (264, 9), (32, 10)])
def test_conv_c1_rejects(gpu, fout, noff):
    kf = gpu
    dt, dh = [0] * noff, list(range(noff))
    T, h = 2, 12
    dx, dw = up_u16(kf, np.zeros((T, h), np.float16)), up_u16(kf, np.zeros((10, 264), np.float16))
    dy = up_u16(kf, poison16(T * h, 264))
    dW, db = up_u32(kf, poison32(10 * 264)), up_u32(kf, poison32(264))
    rc = kf.core.kf_conv_c1_forward(T, h, h, 1, fout, noff, iarr(dt), iarr(dh), dx.ptr, dw.ptr, None, None, None,
                                    dy.ptr, None)
    rejected(kf, rc, f"conv_c1_forward: noff={noff} fout={fout}")
    rc = kf.core.kf_conv_c1_wgrad(T, h, h, 1, fout, noff, iarr(dt), iarr(dh), dx.ptr, dy.ptr, dW.ptr, db.ptr)
    rejected(kf, rc, f"conv_c1_wgrad: noff={noff} fout={fout}")
    kf.sync()
    assert np.all(rd_u16(kf, dy.ptr, (T * h, 264)) == NAN16)
    assert np.all(rd_u32(kf, dW.ptr, (10 * 264,)) == POISON32) and np.all(rd_u32(kf, db.ptr, (264,)) == POISON32)


# ---------------------------------------------------------------- kf_sgd_flat / kf_f32_to_f16_flat
SGD_N = [1, 3, 4, 5, 4099]


def _run_sgd(kf, w0, g, v0, lr, mom, n):
    pad = 8
    tot = len(w0) + pad

    def img(a):
        o = poison32(tot)
        o[:len(a)] = np.asarray(a, np.float32).view(np.uint32)
        return o
    dw, dg, dv = up_u32(kf, img(w0)), up_u32(kf, img(g)), up_u32(kf, img(v0))
    dh = up_u16(kf, poison16(1, tot))
    kf.check(kf.core.kf_sgd_flat(dw.ptr, dh.ptr, dg.ptr, dv.ptr, float(lr), float(mom), n), "sgd_flat")
    kf.sync()
    w, v, h = rd_u32(kf, dw.ptr, (tot,)), rd_u32(kf, dv.ptr, (tot,)), rd_u16(kf, dh.ptr, (tot,))
    assert np.array_equal(w[n:], img(w0)[n:]) and np.array_equal(v[n:], img(v0)[n:]) and np.all(h[n:] == NAN16)
    assert np.array_equal(rd_u32(kf, dg.ptr, (tot,)), img(g))
    return w[:n].view(np.float32), v[:n].view(np.float32), h[:n].view(np.float16)


@pytest.mark.parametrize("n", SGD_N)
def test_sgd_flat(gpu, n):
    kf = gpu
    rng = np.random.default_rng(n)
    w0, g, v0 = gauss(rng, n, np.float32), gauss(rng, n, np.float32), gauss(rng, n, np.float32)
    lr, mom = np.float32(0.05), np.float32(0.9)
    w, v, h = _run_sgd(kf, w0, g, v0, lr, mom, n)
    _, v_ref = R.sgd_flat(w0, g, v0, lr, mom)
    within(v, v_ref, 2.0 ** -23 * (np.abs(float(mom) * R.f64(v0)) + np.abs(R.f64(g))))
    w_ref, _ = R.sgd_flat(w0, v, 0.0, lr, 0.0)      # w0 - lr * v_read
    within(w, w_ref, 2.0 ** -23 * (np.abs(R.f64(w0)) + np.abs(float(lr) * R.f64(v))))
    assert np.array_equal(h.view(np.uint16), w.astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("n", SGD_N)
def test_sgd_flat_w16_rounds_the_stored_w32(gpu, n):
    """w16 = rne(w32), two roundings: updates whose exact value lies 2^-40 beside an fp16 tie
    round to the tie in fp32 and from there to even, where one rounding of the exact value
    goes the other way (every element, so also the n % 4 tail)"""
    kf = gpu
    i = np.arange(n)
    w0 = np.where(i % 2 == 0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11).astype(np.float32)
    g = np.where(i % 2 == 0, -(2.0 ** -40), 2.0 ** -40).astype(np.float32)
    v0 = gauss(np.random.default_rng(n), n, np.float32)
    w, v, h = _run_sgd(kf, w0, g, v0, np.float32(1.0), np.float32(0.0), n)
    assert np.array_equal(v, g) and np.array_equal(w, w0)
    want = np.where(i % 2 == 0, 1.0, 1 + 2.0 ** -9).astype(np.float16)
    assert np.array_equal(w.astype(np.float16), want)
    assert np.array_equal(h.view(np.uint16), want.view(np.uint16))


_F16_EDGES = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504.0, 65520.0, 65519.996, 1e-8, 2.0 ** -24, 2.0 ** -25,
                       1.5 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, 1023 * 2.0 ** -24, 3.3 * 2.0 ** -24, 0.0, -0.0,
                       np.inf, -np.inf, np.nan, -65520.0, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23], np.float32)


@pytest.mark.parametrize("n", [1, 7, 4099])
def test_f32_to_f16_flat(gpu, n):
    kf = gpu
    rng = np.random.default_rng(n)
    pool = np.concatenate([_F16_EDGES, gauss(rng, 4099 - len(_F16_EDGES), np.float32) *
                           (2.0 ** rng.integers(-20, 16, 4099 - len(_F16_EDGES))).astype(np.float32)])
    dsrc = up_u32(kf, pool)
    starts = range(len(_F16_EDGES)) if n == 1 else (0, 7, 14) if n == 7 else (0,)
    for s in starts:
        ddst = up_u16(kf, poison16(1, n + 8))
        kf.check(kf.core.kf_f32_to_f16_flat(dsrc.ptr + 4 * s, ddst.ptr, n), "f32_to_f16_flat")
        kf.sync()
        out = rd_u16(kf, ddst.ptr, (n + 8,))
        assert np.all(out[n:] == NAN16)
        with np.errstate(over="ignore"):
            ref = pool[s:s + n].astype(np.float16)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(out[:n].view(np.float16)), nan)
        assert np.array_equal(out[:n][~nan], ref.view(np.uint16)[~nan])


# ---------------------------------------------------------------- row sets
def _row_cases(T):
    full = (T - 1) // 3 + 1
    for tc0 in (full, full - 9):
        for nt in ((0,) if (T - 1) % 3 == 0 else (0, 1, 5)):
            yield tc0, tc0 + nt


@pytest.mark.parametrize("row_bytes", [16, 48, 528])
@pytest.mark.parametrize("T", [100, 101, 102])
def test_gather_scatter_rows(gpu, T, row_bytes):
    kf = gpu
    rng = np.random.default_rng(T + row_bytes)
    w = row_bytes // 2
    src = rng.integers(1, 0x7C00, (T, w)).astype(np.uint16)      # nonzero words, none the poison
    dsrc = up_u16(kf, src)
    for tc0, tc in _row_cases(T):
        dcomp = up_u16(kf, poison16(tc + 2, w))
        kf.check(kf.core.kf_gather_rows(dcomp.ptr, dsrc.ptr, row_bytes, T, tc0, tc), "gather_rows")
        kf.sync()
        comp = rd_u16(kf, dcomp.ptr, (tc + 2, w))
        check_padding(comp, tc, w, NAN16)
        assert np.array_equal(comp[:tc], R.gather_rows(src, T, tc0, tc))
        y = comp[:tc]
        for r0 in (None, 0, 1, 50, T - 1):      # None: kf_scatter_rows
            n = T - (r0 or 0)
            dfull = up_u16(kf, poison16(n + 2, w))
            if r0 is None:
                rc = kf.core.kf_scatter_rows(dfull.ptr, dcomp.ptr, row_bytes, T, tc0, tc)
            else:
                rc = kf.core.kf_scatter_rows_from(dfull.ptr, dcomp.ptr, row_bytes, T, tc0, tc, r0)
            kf.check(rc, "scatter_rows")
            kf.sync()
            fullrows = rd_u16(kf, dfull.ptr, (n + 2, w))
            check_padding(fullrows, n, w, NAN16)
            assert np.array_equal(fullrows[:n], R.scatter_rows(y, T, tc0, tc, r0 or 0))
            if not r0:      # gather(scatter(y)) == y, on the device
                dback = up_u16(kf, poison16(tc, w))
                kf.check(kf.core.kf_gather_rows(dback.ptr, dfull.ptr, row_bytes, T, tc0, tc), "gather_rows")
                kf.sync()
                assert np.array_equal(rd_u16(kf, dback.ptr, (tc, w)), y)


@pytest.mark.parametrize("row_bytes,T,tc0,tc,r0,why", [
    (24, 10, 2, 3, 0, "row_bytes % 16"),
    (16, 10, 3, 2, 0, "tc < tc0"),
    (16, 10, 5, 5, 0, "3(tc0-1) > T-1"),
    (16, 10, 2, 3, 10, "r0 = T"),
    (16, 10, 2, 7, 0, "lowest tail row 9 - 3*4 < 0"),
    (16, 4, 1, 4, 0, "lowest tail row 3 - 3*2 < 0 (tc = 3 is the last accepted, below)"),
])
def test_gather_scatter_rows_reject(gpu, row_bytes, T, tc0, tc, r0, why):
    """Bad geometries return -1 and launch nothing. The source pointer sits behind 3*(tc-tc0)
    + 16 rows of slack (and as many follow it), so no geometry tried here could address
    outside the allocation even on a build without the validation."""
    kf = gpu
    w = 16       # words per allocated row: at least row_bytes
    slack = 3 * max(tc - tc0, 0) + 16
    dsrc = up_u16(kf, np.ones((T + 2 * slack, w), np.uint16))
    ddst = up_u16(kf, poison16(T + tc + 16, w))
    p = dsrc.ptr + slack * w * 2
    text = f"bad geometry (row_bytes {row_bytes} T {T} tc0 {tc0} tc {tc}"
    if r0 == 0:
        rejected(kf, kf.core.kf_gather_rows(ddst.ptr, p, row_bytes, T, tc0, tc), "gather_rows: " + text)
        rejected(kf, kf.core.kf_scatter_rows(ddst.ptr, p, row_bytes, T, tc0, tc), "scatter_rows: " + text)
    rejected(kf, kf.core.kf_scatter_rows_from(ddst.ptr, p, row_bytes, T, tc0, tc, r0),
             "scatter_rows: " + text + f" r0 {r0})")
    kf.sync()
    assert np.all(rd_u16(kf, ddst.ptr, (T + tc + 16, w)) == NAN16)


def test_gather_rows_tail_reaching_row_zero(gpu):
    """the longest tail the rule accepts: its lowest row is source row 0 (a head row too)"""
    kf = gpu
    T, tc0, tc = 4, 1, 3
    src = np.arange(1, T * 8 + 1, dtype=np.uint16).reshape(T, 8)
    dsrc, ddst = up_u16(kf, src), up_u16(kf, poison16(tc + 1, 8))
    kf.check(kf.core.kf_gather_rows(ddst.ptr, dsrc.ptr, 16, T, tc0, tc), "gather_rows")
    kf.sync()
    out = rd_u16(kf, ddst.ptr, (tc + 1, 8))
    assert R.compact_rows(T, tc0, tc).tolist() == [0, 0, 3]
    assert np.array_equal(out[:tc], src[[0, 0, 3]]) and np.all(out[tc:] == NAN16)


# ---------------------------------------------------------------- row sums
def _mixed_scale(rng, shape):
    """Gaussian fp16 values over many binades, so that fp32 partial sums round and the order
    of the sum shows"""
    return (rng.standard_normal(shape) * 2.0 ** rng.integers(-12, 5, shape)).astype(np.float16)


@pytest.mark.parametrize("cols", [1, 255, 256, 257])
def test_rows_sum_list(gpu, cols):
    kf = gpu
    rng = np.random.default_rng(cols)
    ld = cols + 3
    src = _mixed_scale(rng, (6, cols))
    dsrc = up_u16(kf, padded(src, ld))
    for rows in ([], [2], [4, 1], [3, 0, 3, 5]):
        dedge = up_u16(kf, poison16(1, cols + 8))
        kf.check(kf.core.kf_rows_sum_list(dedge.ptr, dsrc.ptr, ld, iarr(rows), len(rows), cols), "rows_sum_list")
        kf.sync()
        out = rd_u16(kf, dedge.ptr, (cols + 8,))
        assert np.all(out[cols:] == NAN16)
        assert np.array_equal(out[:cols], R.rows_sum(src, rows).view(np.uint16)), rows
    dedge = up_u16(kf, poison16(1, cols + 8))
    rejected(kf, kf.core.kf_rows_sum_list(dedge.ptr, dsrc.ptr, ld, iarr([0, 1, 2, 3, 4]), 5, cols),
             "rows_sum_list: 5 rows")
    kf.sync()
    assert np.all(rd_u16(kf, dedge.ptr, (cols + 8,)) == NAN16)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("cols", [8, 257])
def test_rows_sum(gpu, cols, masked):
    kf = gpu
    rng = np.random.default_rng(cols + masked)
    nrows, ld = 20, cols + 5
    src = _mixed_scale(rng, (nrows, ld))        # the padding columns hold data too: never summed
    mask = rng.integers(0, 2, (nrows, ld)).astype(bool)
    dsrc, dmask = up_u16(kf, src), up_bytes(kf, R.pack_bits(mask))
    for r0, r1 in ((0, 1), (3, 20), (5, 5)):
        dedge = up_u16(kf, poison16(1, cols + 8))
        if masked:
            rc = kf.core.kf_rows_sum_mask(dedge.ptr, dsrc.ptr, ld, r0, r1, cols, dmask.ptr)
        else:
            rc = kf.core.kf_rows_sum(dedge.ptr, dsrc.ptr, ld, r0, r1, cols)
        kf.check(rc, "rows_sum")
        kf.sync()
        out = rd_u16(kf, dedge.ptr, (cols + 8,))
        assert np.all(out[cols:] == NAN16)
        ref = R.rows_sum(src[:, :cols], range(r0, r1), mask[:, :cols] if masked else None)
        assert np.array_equal(out[:cols], ref.view(np.uint16)), (r0, r1)
        if r0 == r1:
            assert np.all(out[:cols] == 0)
