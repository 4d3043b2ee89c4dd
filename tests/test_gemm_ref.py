"""tests/gemm_ref.py itself: the order of the epilogue rule on a hand-worked example, the bit
packing, the MXFP8 acceptance rule, the case tables, and the condition the GPU tests rest on:
with the cases' inputs the error bound leaves at most 0.5 % of the ReLU bits open."""
import numpy as np
import pytest

import gemm_ref as gr
from mx_ref import mx_quantize


def test_epilogue_order_hand_worked():
    """2 x 8, every term on, all values exact in binary. Column 0 pins the order: the bias flips
    the sign before the ReLU (2*1 + 0.5*2 - 4 = -1: bit 0), BN acts on the ReLU's zero
    (0*2 + 1 = 1, not relu(-1*2 + 1) = 0), the residual comes after BN (1 + 0.5*2 = 2, not
    (0 + 1)*2 + 1 = 3). Row 1, column 4: v = 1 + 2^-11 is no fp16 value, and out2 carries it."""
    e = 2.0 ** -11
    acc = np.array([[1, -1, 0.5, -0.25, 2, -2, 0, 3], [3, 0, 0, 0, e, 0, 0, 0]])
    old = np.array([[2, 2, -4, 1, 0, 6, -2, -8], [0] * 8], np.float16)
    bias = np.array([-4, 2, 0.5, 0.25, 0, 1, 2, -1], np.float16)
    scale = np.array([2, 2, -1, 4, 0.5, 3, 1, -2], np.float32)
    shift = np.array([1, -1, 0.5, 0, 1, -2, 0, 3], np.float32)
    resid = np.array([[2, -2, 1, 0, 4, 2, -6, 8], [0] * 8], np.float16)
    scale2 = np.array([1, 3, 2, -1, 0.5, 2, 0.25, 1], np.float32)
    mask_in = np.array([[1, 1, 0, 1, 1, 1, 1, 0], [1] * 8], bool)
    mag = np.ones((2, 8))
    r = gr.epilogue_ref(acc, mag, 2, alpha=2.0, beta=0.5, old=old, bias=bias, relu=True, scale=scale, shift=shift,
                        resid=resid, resid_alpha=0.5, scale2=scale2, mask_in=mask_in)
    pre = np.array([[-1, 1, -0.5, 0.25, 4, 0, 1, 1], [2, 2, 0.5, 0.25, 2 * e, 1, 2, -1]])
    np.testing.assert_array_equal(r["pre"], pre)
    np.testing.assert_array_equal(r["bits"], [[0, 1, 0, 1, 1, 0, 1, 1], [1, 1, 1, 1, 1, 1, 1, 0]])
    np.testing.assert_array_equal(r["v"], [[2, 0, 1, 1, 5, -1, -2, 5], [5, 3, 0, 1, 1 + e, 1, 2, 3]])
    np.testing.assert_array_equal(r["out2"], [[2, 0, 0, -1, 2.5, -2, -0.5, 0], [5, 9, 0, -1, 0.5 + e / 2, 2, 0.5, 3]])
    assert np.float16(r["v"][1, 4]) == 1.0 and r["out2"][1, 4] != 0.5
    # the bound: |alpha| K 2^-23 mag + 1e-6 |pre| at the pre-activation, then |scale|, |scale2|, the mask
    b0 = 2 * 2 * gr.U23 + 1e-6 * np.abs(pre)
    np.testing.assert_allclose(r["bound"], b0 * np.abs(scale), rtol=1e-15)
    np.testing.assert_allclose(r["bound2"], b0 * np.abs(scale) * np.abs(scale2) * mask_in, rtol=1e-15)
    np.testing.assert_allclose(r["tol"], r["bound"] + np.abs(r["v"]) * 2.0 ** -10 + 2.0 ** -24, rtol=1e-15)
    # pre = 0 exactly is inside the bound, like every |pre| <= bound
    assert not r["sure"][0, 5] and r["sure"][0, 0]


def test_epilogue_terms_are_optional():
    acc = np.array([[1.5, -2.0]])
    r = gr.epilogue_ref(acc, np.abs(acc), 8, alpha=0.5)
    np.testing.assert_array_equal(r["v"], [[0.75, -1.0]])
    np.testing.assert_array_equal(r["out2"], r["v"])
    assert r["bits"] is None and r["sure"] is None


def test_bit_packing_linear_order_with_leading_dimension():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2, (5, 16)).astype(bool)
    pad = rng.integers(0, 2, (5, 8)).astype(bool)
    buf = gr.pack_bits(bits, 24, pad)
    assert buf.size == 15
    for m, n in ((0, 0), (0, 15), (3, 7), (4, 9)):
        i = m * 24 + n
        assert bool((buf[i >> 3] >> (i & 7)) & 1) == bits[m, n]
    full = gr.unpack_bits(buf, 5, 24)
    np.testing.assert_array_equal(full[:, :16], bits)
    np.testing.assert_array_equal(full[:, 16:], pad)
    assert not gr.unpack_bits(gr.pack_bits(bits, 24), 5, 24)[:, 16:].any()


def test_splice_policies_and_edge_row():
    x = np.arange(12.0).reshape(6, 2)   # 4 rows + 2 spare
    rows = np.arange(4)
    c = gr.splice(x, rows, (-1, 0), gr.KF_CLAMP)
    np.testing.assert_array_equal(c[:, 0], [0, 0, 2, 4])
    np.testing.assert_array_equal(c[:, 2:], x[:4])
    z = gr.splice(x, rows, (2, 0), gr.KF_ZERO, edges=((0, 0, 4),))
    np.testing.assert_array_equal(z[:, 0], [8, 6, 0, 0])   # row 0 reads the spare row 4


def test_mx_acceptance_rule():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((4, 64)) * 3
    q, s = mx_quantize(v)
    v32 = v.astype(np.float32).astype(np.float64)
    bs, bc = gr.mx_mismatch(q, s, v32, np.zeros_like(v))
    assert not bs.any() and not bc.any()
    q2 = q.copy()
    q2[1, 5] ^= 1     # a neighbouring code, far from a rounding boundary in general
    assert gr.mx_mismatch(q2, s, v32, np.full_like(v, 1e-7))[1][1, 5]
    assert not gr.mx_mismatch(q2, s, v32, np.full_like(v, 0.5))[1].any()
    s2 = s.copy()
    s2[0, 0] += 1
    assert gr.mx_mismatch(q, s2, v32, np.full_like(v, 1e-7))[0][0, 0]


def test_case_tables_name_every_tile():
    fused = gr.fused_cases()
    assert {c["tile"] for c in fused} == set(gr.TILE_SHAPES)
    assert len({c["id"] for c in fused}) == len(fused)
    for c in fused:
        assert c["N"] % 8 == 0 and c["K"] % 8 == 0
        if c["epi"] not in ("mx0", "mx1") and not c["masked"] and c["K"] not in (640, 648):
            assert c["M"] % c["tile"][0] and c["K"] % 64, c["id"]
            # the 160- and 192-column tiles are only chosen for whole column tiles
            assert c["N"] % c["tile"][1] or c["tile"][1] in (160, 192), c["id"]
    wg = gr.wgrad_cases()
    assert {c["tile"] for c in wg} == set(gr.WGRAD_TILES)
    assert len({c["id"] for c in wg}) == len(wg)


_SHAPES = [c for c in gr.fused_cases() if c["epi"] in ("fwd", "mx0", "mx1")]   # every case with a ReLU


@pytest.mark.parametrize("case", _SHAPES, ids=[c["id"] for c in _SHAPES])
def test_relu_ambiguity_share(case):
    """The GPU test exempts a ReLU bit where |pre-activation| <= bound. From the reference alone:
    that is at most 0.5 % of a case's elements (0.004 % to 0.09 % for K = 72 to 648 with
    unit-normal A, B ~ N(0, 1/K) and bias in +-0.5). The 36,490-row case checks a sample."""
    d = gr.fused_inputs(case)
    rows = None
    if case["M"] > 30000:
        rows = np.random.default_rng(1).choice(case["M"], 4096, replace=False)
    share = gr.relu_exempt_share(d["ref"], rows)
    print("exempt share %s: %.5f %%" % (case["id"], 100 * share))
    assert share <= 0.005
