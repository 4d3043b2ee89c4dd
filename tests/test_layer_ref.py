"""The plain references of tests/layer_ref.py checked against each other on the CPU, before
a GPU test compares a kernel with them: each backward is the transpose of its forward, the
row-set scatter inverts the gather, and the two independent conv restatements (direct taps
and im2col) agree."""
import numpy as np
import pytest

import layer_ref as R


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape).astype(np.float64)


SMALL_GEOMS = [  # (T, hin, hout, sub, fin, dts, dhs, kp)
    (1, 5, 5, 1, 1, R.T3, R.T3, 16),
    (23, 10, 10, 1, 3, R.T3, R.T3, 32),
    (23, 10, 5, 2, 6, R.T3, R.T3, 64),
    (7, 9, 4, 2, 8, (0, 1), (0,), 16),
    (23, 12, 6, 2, 3, (0,), (1, 2), 8),
]


@pytest.mark.parametrize("geom", SMALL_GEOMS)
def test_im2col_col2im_adjoint(geom):
    T, hin, hout, sub, fin, dts, dhs, kp = geom
    dt, dh = R.taps(dts, dhs)
    rng = np.random.default_rng(1)
    x = _ints(rng, (T, hin * fin), -5, 5)
    P = _ints(rng, (T * hout, kp), -5, 5)
    lhs = np.sum(R.im2col_small(x, T, hin, hout, sub, fin, dt, dh, kp) * P)
    P[:, len(dt) * fin:] = 0     # col2im reads only the columns im2col fills
    rhs = np.sum(x * R.col2im_small(P, T, hin, hout, sub, fin, dt, dh, kp))
    assert lhs == rhs and lhs != 0


def test_im2col_padding_columns_zero():
    dt, dh = R.taps(R.T3, R.T3)
    x = np.ones((4, 6 * 6))
    P = R.im2col_small(x, 4, 6, 6, 1, 6, dt, dh, 64)
    assert np.all(P[:, 54:] == 0) and P[1 * 6 + 2, :54].min() == 1


@pytest.mark.parametrize("geom", R.C1_GEOMS)
def test_conv_c1_adjoint_and_im2col(geom):
    T, hin, hout, sub, fout, dts, dhs = geom
    dt, dh = R.taps(dts, dhs)
    rng = np.random.default_rng(2)
    x = _ints(rng, (T, hin), -3, 3)
    W = _ints(rng, (len(dt), fout), -2, 2)
    b = _ints(rng, fout, -4, 4)
    dz = _ints(rng, (T * hout, fout), -2, 2)
    pre, mask, y = R.conv_c1(x, W, b, None, None, T, hin, hout, sub, dt, dh)
    dW, db = R.conv_c1_wgrad(x, dz, T, hin, hout, sub, dt, dh)
    assert np.sum(pre * dz) == np.sum(W * dW) + np.sum(b * db)
    # the same conv as im2col (one input filter) times W
    P = R.im2col_small(x, T, hin, hout, sub, 1, dt, dh, 16)[:, :len(dt)]
    assert np.array_equal(pre, P @ W + b)
    assert np.array_equal(mask, pre > 0) and np.array_equal(y, np.maximum(pre, 0))
    assert (pre == 0).mean() > 0.001    # integer data puts exact zeros at the ReLU


def test_conv_c1_scale_shift():
    dt, dh = R.taps((0,), (0,))
    x = np.array([[1.0, -2.0]])
    pre, mask, y = R.conv_c1(x, [[3.0]], [0.5], [2.0], [-1.0], 1, 2, 2, 1, dt, dh)
    assert pre.ravel().tolist() == [3.5, -5.5] and mask.ravel().tolist() == [True, False]
    assert y.ravel().tolist() == [6.0, -1.0]


@pytest.mark.parametrize("geom", R.C1_GEOMS)
def test_conv_c1_gaussian_mask_skip_share(geom):
    """the share of elements whose pre-activation lies inside the fp32 accumulation bound
    (where the GPU test cannot demand a mask bit) stays far below 0.1 %"""
    T, hin, hout, sub, fout, dts, dhs = geom
    dt, dh = R.taps(dts, dhs)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((T, hin)).astype(np.float16)
    W = rng.standard_normal((len(dt), fout)).astype(np.float16)
    b = rng.standard_normal(fout).astype(np.float16)
    pre, _, _ = R.conv_c1(x, W, b, None, None, T, hin, hout, sub, dt, dh)
    S, _, _ = R.conv_c1(np.abs(x), np.abs(W), np.abs(b), None, None, T, hin, hout, sub, dt, dh)
    inside = np.abs(pre) <= (len(dt) + 1) * R.F32_U * S
    assert inside.mean() <= 1e-4


@pytest.mark.parametrize("T", [100, 101, 102])
def test_gather_inverts_scatter(T):
    rng = np.random.default_rng(T)
    full = (T - 1) // 3 + 1
    for tc0 in (full, full - 7):
        for nt in ((0,) if (T - 1) % 3 == 0 else (0, 1, 5)):
            tc = tc0 + nt
            rows = R.compact_rows(T, tc0, tc)
            assert len(set(rows.tolist())) == tc and rows.min() >= 0 and rows.max() <= T - 1
            if nt:
                assert rows[-1] == T - 1 and rows[tc0] == T - 1 - 3 * (nt - 1)
            y = rng.integers(1, 100, (tc, 4))
            full_rows = R.scatter_rows(y, T, tc0, tc)
            assert np.array_equal(R.gather_rows(full_rows, T, tc0, tc), y)
            assert np.count_nonzero(full_rows.any(axis=1)) == tc
            for r0 in (1, 50, T - 1):
                assert np.array_equal(R.scatter_rows(y, T, tc0, tc, r0), full_rows[r0:])


@pytest.mark.parametrize("nf1", [0, 3])
def test_combine_bwd_is_transpose(nf1):
    T, height, nf2 = 50, 7, 2
    seq_off = [0, 10, 10, 37, 50]
    rng = np.random.default_rng(5)
    a = _ints(rng, (T, height * nf1), -5, 5)
    b = _ints(rng, (4, height * nf2), -5, 5)
    dy = _ints(rng, (T, height * (nf1 + nf2)), -5, 5)
    out = R.combine_fm(a, b, seq_off, T, height, nf1, nf2)
    da = dy.reshape(T, height, nf1 + nf2)[:, :, :nf1].reshape(T, -1)
    assert np.sum(out * dy) == np.sum(a * da) + np.sum(b * R.combine_fm_bwd(dy, seq_off, height, nf1, nf2))
    assert np.all(R.combine_fm_bwd(dy, seq_off, height, nf1, nf2)[1] == 0)     # the empty sequence
    # frame-level b: every frame its own row
    bt = _ints(rng, (T, height * nf2), -5, 5)
    o2 = R.combine_fm(a, bt, None, T, height, nf1, nf2).reshape(T, height, nf1 + nf2)
    assert np.array_equal(o2[:, :, nf1:].reshape(T, -1), bt) and np.array_equal(o2[:, :, :nf1].reshape(T, -1), a)


def test_rows_sum_order_and_mask():
    # fp32 sequential: 2048 + 1 + 1 ... in fp16 steps would stall; in fp32 it does not
    src = np.array([[2048.0], [1.0], [1.0], [-2048.0]], np.float16)
    assert R.rows_sum(src, [0, 1, 2, 3])[0] == 2.0
    assert R.rows_sum(src, [0, 1, 2])[0] == np.float16(2050.0)
    assert R.rows_sum(src, [])[0] == 0.0 and R.rows_sum(src, [1, 1, 1])[0] == 3.0
    m = np.array([[True], [False], [True], [True]])
    assert R.rows_sum(src, [0, 1, 2, 3], m)[0] == 1.0
    # every step rounds to fp32: 2^11 + 2^-13 is a tie there and goes back to 2^11, twice;
    # the other order adds 2^-12 exactly
    s2 = np.array([[2048.0], [2.0 ** -13], [2.0 ** -13], [-2048.0]], np.float16)
    assert R.rows_sum(s2, [0, 1, 2, 3])[0] == 0.0
    assert R.rows_sum(s2, [1, 2, 0, 3])[0] == np.float16(2.0 ** -12)


def test_pack_bits_roundtrip():
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2, 77).astype(bool)
    p = R.pack_bits(bits)
    assert p.dtype == np.uint8 and len(p) == 10
    assert np.array_equal(R.unpack_bits(p, 77), bits)
    one = np.zeros(16, bool)
    one[9] = True
    assert R.pack_bits(one).tolist() == [0, 2]


def test_sgd_flat():
    w, v = R.sgd_flat([1.0, 2.0], [0.5, -1.0], [2.0, 4.0], 0.25, 0.5)
    assert v.tolist() == [1.5, 1.0] and w.tolist() == [0.625, 1.75]


def test_acc_bound_forms():
    assert R.acc_bound(4, 2.0) == 4 * 2.0 ** -24 * 2.0 + 2.0 ** -24
    assert R.acc_bound(4, 2.0, -8.0) == R.acc_bound(4, 2.0) + 8.0 * 2.0 ** -10
