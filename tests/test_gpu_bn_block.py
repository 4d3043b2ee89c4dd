"""Block statistics of the training-mode BatchNorm (kf_ops.h kf_bn_block_stats /
kf_bn_block_bwd_stats, the maskless kf_bn_train_bwd_apply) against float64. The
bounds are test_gpu_bn_train.py's for the same quantities: fp32 stores of double sums."""
import numpy as np
import pytest

import bn_sites_ref as bs

pytestmark = pytest.mark.gpu

EPS = 1e-3
U24, U23 = 2.0 ** -24, 2.0 ** -23
ROWS_PER_WG = 64   # kBlkRows in kaldi-fp16_amd/csrc/batchnorm.hip: the tensor rows a workgroup takes

# (rows, H, F, ld): one lane group; odd H; the three conv widths of cnn_tdnn_17f; ld > H F; one
# below, at and one above a workgroup's rows; five workgroups and a remainder with a block width
# whose lane groups do not divide the workgroup (F / 8 = 3); two column slabs (F / 8 > 256)
SHAPES = [(1, 1, 8, 8), (7, 3, 8, 24), (65, 40, 32, 1280), (257, 20, 64, 1280), (1031, 10, 128, 1280),
          (131, 10, 256, 2560), (257, 20, 64, 1280 + 64),
          (ROWS_PER_WG - 1, 3, 16, 48), (ROWS_PER_WG, 3, 16, 48), (ROWS_PER_WG + 1, 3, 16, 48),
          (5 * ROWS_PER_WG + 37, 2, 24, 48), (9, 1, 2056, 2056)]


def _r_matrix(rng, rows, H, F):
    """a ReLU output in fp16 whose blocks 0, 1, 2 break naive sums: all zero, constant (var 0),
    mean 4 with standard deviation 1/64"""
    r = np.maximum(rng.standard_normal((rows, H, F)) + 0.3, 0.0)
    r[:, :, 0] = 0.0
    r[:, :, 1] = 2.5
    r[:, :, 2] = 4.0 + rng.standard_normal((rows, H)) / 64.0
    return r.reshape(rows, H * F).astype(np.float16)


def _pad(a, ld, fill):
    out = np.full((a.shape[0], ld), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _f16_ulp(x):
    return np.maximum(np.spacing(np.abs(x).astype(np.float16)).astype(np.float64), 2.0 ** -24)


def _read_f64(kf, buf, n):
    return kf.read_f32(buf.ptr, (2 * n,)).view(np.float64).copy()


SENT = 7.0  # what the 8 floats (2 doubles) behind every [F] output hold before and after


def _stats(kf, rb, ld, rows, H, F, rms, acc):
    """-> [4 x F + 8] mean | var | scale | shift with their sentinels"""
    st = kf.upload_f32(np.full(4 * (F + 8), SENT, np.float32))
    p = lambda k: st.ptr + 4 * (F + 8) * k
    ap = (acc.ptr, acc.ptr + 16, acc.ptr + 16 + 8 * (F + 2)) if acc is not None else (None, None, None)
    kf.check(kf.core.kf_bn_block_stats(rb.ptr, ld, rows, H, F, EPS, rms, p(0), p(1), p(2), p(3), *ap), "kf_bn_block_stats")
    return st, kf.read_f32(st.ptr, (4, F + 8))


@pytest.mark.parametrize("rows,H,F,ld", SHAPES)
def test_forward_against_float64(gpu, rows, H, F, ld):
    kf = gpu
    rng = np.random.default_rng(rows * 7 + H * 3 + F)
    rms = 0.75
    r16 = _r_matrix(rng, rows, H, F)
    r = r16.astype(np.float64)
    ref = bs.bn_block_forward(r, H, F, EPS, rms)
    rv = r.reshape(rows * H, F)
    rb = kf.upload_fp16(_pad(r16, ld, 7))                  # (the pad columns must not be read)
    acc = kf.upload_f32(np.concatenate([np.zeros(2), np.zeros(F), [SENT] * 2, np.zeros(F), [SENT] * 2]).view(np.float32))
    st, stats = _stats(kf, rb, ld, rows, H, F, rms, acc)
    assert np.all(stats[:, F:] == SENT)                    # nothing past F is written
    mean, var, scale, shift = (s[:F].astype(np.float64) for s in stats)
    er2 = (rv * rv).mean(0)
    print("mean err / bound %.3g" % np.max(np.abs(mean - ref["mean"]) / (U23 * np.abs(ref["mean"]) + 1e-300)))
    assert np.all(np.abs(mean - ref["mean"]) <= U23 * np.abs(ref["mean"]))
    bvar = U23 * ref["var"] + 1e-12 * er2
    assert np.all(np.abs(var - ref["var"]) <= bvar)
    assert var[0] == 0.0 and var[1] == 0.0 and np.all(var >= 0)
    bsc = U23 * ref["scale"] + 0.5 * ref["scale"] * (1e-12 * er2) / (ref["var"] + EPS)
    assert np.all(np.abs(scale - ref["scale"]) <= bsc)
    bsh = U23 * np.abs(ref["shift"]) + np.abs(ref["mean"]) * bsc
    assert np.all(np.abs(shift - ref["shift"]) <= bsh)
    # the accumulators took this batch: count = rows H, the double sums
    n_acc = 2 + 2 * (F + 2)
    a = _read_f64(kf, acc, n_acc)
    assert a[0] == rows * H
    s_acc, q_acc = a[2:2 + F], a[2 + F + 2:2 + F + 2 + F]
    assert np.all(np.abs(s_acc - rv.sum(0)) <= 1e-12 * np.abs(rv).sum(0))
    assert np.all(np.abs(q_acc - (rv * rv).sum(0)) <= 1e-12 * (rv * rv).sum(0))
    assert np.all(a[2 + F:2 + F + 2] == SENT) and np.all(a[-2:] == SENT)
    # bit for bit on a second run; the accumulators add up
    _, stats2 = _stats(kf, rb, ld, rows, H, F, rms, acc)
    assert np.array_equal(stats.view(np.uint32), stats2.view(np.uint32))
    a2 = _read_f64(kf, acc, n_acc)
    assert a2[0] == 2 * rows * H and np.array_equal(a2[2:2 + F], 2 * s_acc)
    # without accumulators: the same statistics
    _, stats3 = _stats(kf, rb, ld, rows, H, F, rms, None)
    assert np.array_equal(stats.view(np.uint32), stats3.view(np.uint32))
    if ld != H * F:
        return
    # the apply through the dense [rows H x F] view: one fp16 ulp, the statistics' error carried
    # through, and the fp32 rounding of the epilogue's fmaf
    ob = kf.upload_fp16(np.full((rows * H, F), 9, np.float16))
    p = lambda k: st.ptr + 4 * (F + 8) * k
    kf.check(kf.core.kf_bn_train_apply(rb.ptr, F, rows * H, F, p(2), p(3), None, 0, None, None, 0, 0.0, ob.ptr, F),
             "kf_bn_train_apply")
    out = kf.read_fp16(ob.ptr, (rows, H * F)).astype(np.float64)
    tol = _f16_ulp(ref["out"]) + np.abs(r) * np.tile(bsc, H) + np.tile(bsh, H) + \
        3 * U24 * (np.abs(r * np.tile(ref["scale"], H)) + np.abs(np.tile(ref["shift"], H)))
    err = np.abs(out - ref["out"])
    print("out err / tol max %.3g" % np.max(err / tol))
    assert np.all(err <= tol)


@pytest.mark.parametrize("rows,H,F,ld", SHAPES)
def test_backward_against_float64(gpu, rows, H, F, ld):
    kf = gpu
    rng = np.random.default_rng(rows * 11 + H * 5 + F)
    rms = 0.75
    r16 = _r_matrix(rng, rows, H, F)
    g16 = (rng.standard_normal((rows, H * F)) * 0.1).astype(np.float16)
    r, g = r16.astype(np.float64), g16.astype(np.float64)
    fwd = bs.bn_block_forward(r, H, F, EPS, rms)
    sc32, sh32 = fwd["scale"].astype(np.float32), fwd["shift"].astype(np.float32)
    sc, sh = sc32.astype(np.float64), sh32.astype(np.float64)   # the reference on the kernel's own inputs
    a_ref, b_ref, gr = bs.bn_block_backward(g, r, H, F, sc, sh, rms)
    gb, rb = kf.upload_fp16(_pad(g16, ld, 5)), kf.upload_fp16(_pad(r16, ld, 7))
    scb, shb = kf.upload_f32(sc32), kf.upload_f32(sh32)
    ab = kf.upload_f32(np.full(2 * (F + 8), SENT, np.float32))
    pa, pb = ab.ptr, ab.ptr + 4 * (F + 8)

    def stats():
        kf.check(kf.core.kf_bn_block_bwd_stats(gb.ptr, ld, rb.ptr, ld, rows, H, F, scb.ptr, shb.ptr, rms, pa, pb),
                 "kf_bn_block_bwd_stats")
        return kf.read_f32(ab.ptr, (2, F + 8))

    ab1 = stats()
    assert np.all(ab1[:, F:] == SENT)
    a, b = ab1[0, :F].astype(np.float64), ab1[1, :F].astype(np.float64)
    gv, rv = g.reshape(rows * H, F), r.reshape(rows * H, F)
    ba = U23 * np.abs(a_ref) + 1e-12 * np.abs(gv).mean(0)
    bb = U23 * np.abs(b_ref) + 1e-12 * (np.abs(sc) * np.abs(gv * rv).mean(0) + np.abs(sh) * np.abs(gv).mean(0)) / rms
    print("a err / bound %.3g, b err / bound %.3g" % (np.max(np.abs(a - a_ref) / (ba + 1e-300)),
                                                     np.max(np.abs(b - b_ref) / (bb + 1e-300))))
    assert np.all(np.abs(a - a_ref) <= ba)
    assert np.all(np.abs(b - b_ref) <= bb)
    assert np.array_equal(stats().view(np.uint32), ab1.view(np.uint32))
    if ld != H * F:
        return
    # the apply through the dense view: with the ReLU mask, with an all-ones mask, and with none
    n = rows * H
    bits = rng.integers(0, 2, size=(n, F)).astype(np.uint8)

    def apply(mask_bits):
        mb = None
        if mask_bits is not None:
            packed = np.packbits(mask_bits.reshape(-1), bitorder="little")
            mb = kf.upload_f32(np.frombuffer(packed.tobytes() + b"\0" * (-len(packed) % 4), np.float32))
        dzb = kf.upload_fp16(np.full((n, F), 9, np.float16))
        kf.check(kf.core.kf_bn_train_bwd_apply(gb.ptr, F, rb.ptr, F, n, F, scb.ptr, shb.ptr, rms, pa, pb, None, 0, None,
                                               mb.ptr if mb else None, F, dzb.ptr, F), "kf_bn_train_bwd_apply")
        return kf.read_fp16(dzb.ptr, (n, F))

    yhat = (rv * sc + sh) / rms
    grv = gr.reshape(n, F)
    tol = np.abs(sc) * (ba + np.abs(yhat) * bb)
    masked, ones, none = apply(bits), apply(np.ones_like(bits)), apply(None)
    err = np.abs(masked.astype(np.float64) - grv * bits)
    print("dz err / tol max %.3g" % np.max(err / (_f16_ulp(grv * bits) + tol)))
    assert np.all(err <= _f16_ulp(grv * bits) + tol)
    assert np.all(masked[bits == 0] == 0)
    assert np.array_equal(none.view(np.uint16), ones.view(np.uint16))      # relu_bit = 1, bit for bit
    assert np.all(np.abs(none.astype(np.float64) - grv) <= _f16_ulp(grv) + tol)
    assert np.array_equal(apply(None).view(np.uint16), none.view(np.uint16))


def test_argument_checks(gpu):
    kf = gpu
    buf = kf.upload_f32(np.zeros(256, np.float32))
    p = buf.ptr
    st = lambda ld, rows, H, F, acc=(None, None, None): kf.core.kf_bn_block_stats(p, ld, rows, H, F, EPS, 1.0, p, p, p, p, *acc)
    bw = lambda ld, rows, H, F: kf.core.kf_bn_block_bwd_stats(p, ld, p, ld, rows, H, F, p, p, 1.0, p, p)
    assert st(24, 4, 2, 8) == 0 and bw(24, 4, 2, 8) == 0
    for f in (st, bw):
        assert f(24, 4, 2, 12) != 0        # F % 8
        assert f(8, 4, 2, 8) != 0          # ld < H F
        assert f(16, 0, 2, 8) != 0         # rows
        assert f(16, -3, 2, 8) != 0
        assert f(16, 4, 0, 8) != 0         # H
        assert b"kf_bn_block" in kf.core.kf_last_error()
    assert st(16, 4, 2, 8, (p, None, None)) != 0    # one accumulator without the others
    assert st(16, 4, 2, 8, (None, p, p)) != 0
    kf.sync()
