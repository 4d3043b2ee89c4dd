"""The float64 restatement of the semi-orthogonal constraint (tests/ortho_ref.py), checked on
its own: it is the reference of tests/test_gpu_orthonormal.py and is never compared with the
kernel here. Gaussian W / sqrt(K) from a seeded generator, all in float64.
"""
import numpy as np
import pytest

import kfp16  # noqa: F401  (the constraint's entry points exist in this build)
import ortho_ref as R

assert hasattr(kfp16.nnet, "nnet_constrain_orthonormal")


def _apply(w, c, times):
    """`times` applications in float64 (the float32 rounding of the input is skipped)"""
    W = w.astype(np.float64)
    for _ in range(times):
        n = W.shape[1]
        P = W.T @ W
        tP, tPP = np.trace(P), np.sum(P * P)
        nu = 0.125
        if c < 0:
            s = np.sqrt(tPP / tP)
            ratio = tPP * n / tP ** 2
            nu *= (0.5 if ratio > 1.02 else 1) * (0.5 if ratio > 1.1 else 1)
        else:
            s = c
        W = W - 4 * nu / (s * s) * (W @ (P - s * s * np.eye(n)))
    return W


def _rel_err64(W, c):
    n = W.shape[1]
    P = W.T @ W
    s2 = np.sum(P * P) / np.trace(P) if c < 0 else c * c
    return np.sqrt(np.sum((P - s2 * np.eye(n)) ** 2)) / (s2 * np.sqrt(n))


@pytest.mark.parametrize("K, n", [(32, 32), (256, 64), (416, 96), (3072, 160)])
def test_floating_update_is_orthogonal_to_w(K, n):
    """with the floating scale the update neither grows nor shrinks W to first order"""
    w = R.gaussian(np.random.default_rng(K + n), K, n)
    r = R.ref_constrain(w, -1.0)
    W = w.astype(np.float64)
    assert abs(np.sum(W * r["x"])) <= 1e-12 * np.linalg.norm(W) * np.linalg.norm(r["x"])
    assert np.array_equal(r["w"], W - r["x"]) and r["ratio"] >= 1 - 1e-12


@pytest.mark.parametrize("K, n, c, times", [(256, 64, -1.0, 12), (512, 64, -1.0, 12), (416, 96, -1.0, 12),
                                            (3072, 160, -1.0, 12), (256, 64, 1.0, 12), (512, 64, 0.5, 12),
                                            (32, 32, -1.0, 30)])
def test_repeated_application_converges(K, n, c, times):
    w = R.gaussian(np.random.default_rng(7 * K + n), K, n)
    if c > 0:
        # a fixed scale is met from a matrix near that scale (as Kaldi initialises one): the
        # iteration sigma <- sigma (1 - (sigma^2 / c^2 - 1) / 2) diverges from sigma > sqrt(5) c,
        # which W / sqrt(K) with c = 0.5 reaches (sigma up to 1 + sqrt(n / K))
        w = (np.float32(c) * w).astype(np.float32)
    assert _rel_err64(w.astype(np.float64), c) > 1e-2
    W = _apply(w, c, times)
    assert _rel_err64(W, c) < 1e-12
    # one step of _apply is ref_constrain
    assert np.allclose(_apply(w, c, 1), R.ref_constrain(w, c)["w"], rtol=0, atol=1e-15)


@pytest.mark.parametrize("c", [-1.0, 1.0])
def test_permutation_columns_are_a_fixed_point(c):
    w = R.perm_columns(np.random.default_rng(3), 96, 64)
    r = R.ref_constrain(w, c)
    assert np.array_equal(r["w"], w.astype(np.float64))
    assert (r["s"], r["ratio"], r["err"]) == (1.0, 1.0, 0.0)


def test_scaled_permutation_with_fixed_scale_and_degenerate():
    w = 2 * R.perm_columns(np.random.default_rng(4), 128, 64)
    r = R.ref_constrain(w, 1.0)      # P = 4 I, Q = 3 I, factor 0.5: W - 0.5 * 3 W
    assert np.array_equal(r["w"], -w.astype(np.float64) / 2) and r["nu"] == 0.125 and r["factor"] == 0.5
    z = R.ref_constrain(np.zeros((64, 32), np.float32), -1.0)
    assert z["s"] == 0 and not z["w"].any()
    assert R.ref_constrain(w, 0.0)["s"] == 0


def test_bounds_are_small_against_the_update():
    """the kernel bounds of ortho_ref.kernel_bounds separate a right update from one that is
    2.5 % off (factor 3.9 for 4), at the shapes the GPU test uses"""
    for K, n in [(256, 64), (3072, 160)]:
        w = R.gaussian(np.random.default_rng(K), K, n)
        r = R.ref_constrain(w, -1.0)
        ds, dratio, derr, dw = R.kernel_bounds(w, -1.0, r)
        assert ds < 1e-4 * r["s"] and dratio < 1e-3 * r["ratio"] and derr < 1e-2 * r["err"]
        assert np.mean(0.025 * np.abs(r["x"]) > dw) > 0.5
