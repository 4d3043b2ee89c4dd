"""tests/conv_ref.py itself: the operand rule on a hand-worked example, the residue splits of
the input gradient against the one-piece col2im, the case tables, and the conditions the GPU
tests (tests/test_gpu_conv_halo_elems.py) rest on: the integer data is exact in fp16 / fp32
and not vacuous, and with the Gaussian data the error bound leaves at most 0.5 % of the ReLU
bits open."""
import numpy as np
import pytest

import conv_ref as cr

FWD, DGRAD, WGRAD = cr.forward_cases(), cr.dgrad_cases(), cr.wgrad_cases()


def test_im2col_hand_worked():
    """2 frames of 3 heights, one channel: x = [[1 2 3], [4 5 6]], taps (dt, dh) in row-major
    (-1..1) x (-1..1) order. Row (t, h) holds x[t + dt][h + dh], zero outside either range."""
    x = np.array([[1, 2, 3], [4, 5, 6]], np.float64)
    P = cr.im2col(x, 2, 3, 1, 3, 1, cr.OFFS)
    np.testing.assert_array_equal(P, [[0, 0, 0, 0, 1, 2, 0, 4, 5],
                                      [0, 0, 0, 1, 2, 3, 4, 5, 6],
                                      [0, 0, 0, 2, 3, 0, 5, 6, 0],
                                      [0, 1, 2, 0, 4, 5, 0, 0, 0],
                                      [1, 2, 3, 4, 5, 6, 0, 0, 0],
                                      [2, 3, 0, 5, 6, 0, 0, 0, 0]])
    # height stride 2, two output heights: row (t, h) reads heights 2h + dh
    P2 = cr.im2col(x, 2, 3, 1, 2, 2, cr.OFFS)
    np.testing.assert_array_equal(P2[:2], [[0, 0, 0, 0, 1, 2, 0, 4, 5], [0, 0, 0, 2, 3, 0, 5, 6, 0]])
    # time-strided: one output frame reading source frame t0 + 0 * tmul = 1
    np.testing.assert_array_equal(cr.im2col(x, 2, 3, 1, 3, 1, cr.OFFS, tmul=2, t0=1, nrows=3), P[3:])
    # a padded leading dimension: the pad columns are never read
    xp = np.concatenate([x, np.full((2, 5), 1000.0)], 1)
    np.testing.assert_array_equal(cr.im2col(xp, 2, 3, 1, 3, 1, cr.OFFS, ld=8), P)
    # col2im on the same example: dP of ones counts the taps that reach each input element
    # (frames: 2 of 3 time taps; heights 0 and 2: 2 of 3 height taps, height 1: all 3)
    np.testing.assert_array_equal(cr.col2im(np.ones((6, 9)), 2, 3, 1, 3, 1, cr.OFFS).reshape(2, 3),
                                  [[4, 6, 4], [4, 6, 4]])


@pytest.mark.parametrize("hin,fin,hout,sub", [(6, 2, 6, 1), (6, 2, 3, 2), (10, 1, 5, 2)])
def test_col2im_is_the_transpose(hin, fin, hout, sub):
    rng = np.random.default_rng(hin + sub)
    T = 4
    x = rng.standard_normal((T, hin * fin))
    dP = rng.standard_normal((T * hout, 9 * fin))
    lhs = np.sum(cr.im2col(x, T, hin, fin, hout, sub, cr.OFFS) * dP)
    rhs = np.sum(x.reshape(T * hin, fin) * cr.col2im(dP, T, hin, fin, hout, sub, cr.OFFS))
    assert abs(lhs - rhs) < 1e-10


def test_guarded_layout():
    buf, off = cr.guarded(np.ones((3, 4), np.float16), ld=6)
    assert buf.shape == (7, 6) and off == 12
    assert (buf[2:5, :4] == 1).all() and (buf[:2] == 1000).all() and (buf[5:] == 1000).all() and (buf[:, 4:] == 1000).all()


def test_case_tables():
    for cases in (FWD, DGRAD, WGRAD):
        assert len({c["id"] for c in cases}) == len(cases)
    tiles = {c["geo"][5] * c["geo"][6] for c in FWD}
    assert {1, 2, 8, 9} <= tiles                        # no remap, remap with and without remainder
    assert any(c["geo"][6] == 2 for c in FWD)           # two column tiles
    assert {(c["geo"][2], c["geo"][3]) for c in FWD} >= {(1, 1), (2, 2), (2, 1), (4, 2), (4, 1)}
    for c in FWD:
        hin, fin, hout, sub, fout = c["shape"]
        M = c["nc"] * hout
        assert c["geo"][5] == -(-M // c["geo"][0]) and c["geo"][6] == -(-fout // c["geo"][1]), c["id"]
        assert c["t0"] + (c["nc"] - 1) * c["tmul"] <= c["T"] - 1, c["id"]
    assert any(c["tmul"] == 3 and c["t0"] + (c["nc"] - 1) * 3 == c["T"] - 1 for c in FWD)
    for c in DGRAD:
        calls = cr.dgrad_calls(c)
        assert len(calls) == len(c["geos"])
        for call, g in zip(calls, c["geos"]):
            assert g[5] == -(-call["M"] // g[0]), c["id"]
    assert any(g[5] >= 8 for c in DGRAD if c["kind"] == "plain" for g in c["geos"])
    assert any(g[5] >= 8 for c in DGRAD if c["kind"] == "strided" for g in c["geos"])
    assert {(g[0], g[1], g[2]) for c in WGRAD for g in c["geos"]} == {(64, 4, 3), (64, 4, 2), (128, 8, 2)}
    for c in WGRAD:
        hout = c["shape"][2]
        for (t0, tmul, n), g in zip(cr.wgrad_calls(c), c["geos"]):
            nks = -(-n * hout // 64)
            assert g[3] == -(-nks // g[4]), c["id"]
            if g[3] > 1:
                assert nks % g[4] and (n * hout) % 64 and 64 % hout and 320 % hout == 0 and nks > 5, c["id"]
            assert t0 + (n - 1) * tmul <= c["T"] - 1


@pytest.mark.parametrize("case", FWD, ids=[c["id"] for c in FWD])
def test_forward_case_inputs(case):
    """integer data: every pre-activation an integer of at most 2048 (exact in fp16) and the
    ReLU leaves a fair share of outputs non-zero; Gaussian data: the exempt share under the cap"""
    ref = cr.forward_inputs(case, "int")["ref"]
    pre = ref["pre"]
    assert np.array_equal(pre, np.rint(pre)) and np.abs(pre).max() <= 2048
    assert 0.2 <= np.mean(pre > 0) <= 0.8 and np.mean(pre != 0) > 0.8
    g = cr.forward_inputs(case, "gauss")["ref"]
    share = 1.0 - float(np.mean(g["sure"]))
    print("exempt share %s: %.5f %%" % (case["id"], 100 * share))
    assert share <= cr.RELU_CAP


@pytest.mark.parametrize("case", DGRAD, ids=[c["id"] for c in DGRAD])
def test_dgrad_case_inputs(case):
    """the per-residue GEMMs together are the one-piece col2im of dz . W^T (for the compact
    rows: of a dz that is zero off the compact frames), they own every input row exactly once,
    and the integer data is exact and not vacuous"""
    for data in cr.DATA:
        d = cr.dgrad_inputs(case, data)
        assert d["owned"].all()
        np.testing.assert_allclose(d["out2"], d["whole"], rtol=0, atol=1e-9 * max(1.0, np.abs(d["whole"]).max()))
    d = cr.dgrad_inputs(case, "int")
    for call in d["calls"]:
        pre = call["pre"]
        assert np.array_equal(pre, np.rint(pre)) and np.abs(pre).max() <= 2048
    assert np.array_equal(d["out2"] * 2, np.rint(d["out2"] * 2)) and np.abs(d["out2"]).max() <= 4096
    assert np.mean(d["out2"] != 0) > 0.3


@pytest.mark.parametrize("case", WGRAD, ids=[c["id"] for c in WGRAD])
def test_wgrad_case_inputs(case):
    """integer data: every sum (with the accumulated old value on top, twice) stays an integer
    below 2^24, so fp32 is exact in any split order"""
    d = cr.wgrad_inputs(case, "int")
    tot = np.abs(d["old_w"]).max() + 2 * sum(np.abs(p["acc"]).max() for p in d["parts"])
    assert tot < 2 ** 24
    assert np.abs(d["old_b"]).max() + 2 * sum(np.abs(p["bsum"]).max() for p in d["parts"]) < 2 ** 24
    for p in d["parts"]:
        assert np.array_equal(p["acc"], np.rint(p["acc"])) and np.mean(p["acc"] != 0) > 0.5
        assert max(np.abs(p["mag"]).max(), np.abs(p["bmag"]).max()) < 2 ** 24   # every partial sum too
