"""The float64 restatement of the online natural-gradient preconditioner (tests/natgrad_ref.py),
checked on its own: it is the reference of tests/test_gpu_natgrad.py and is never compared with
the kernels' own output path. No device."""
import numpy as np

import kfp16
import natgrad_ref as R

assert hasattr(kfp16.core, "kf_ng_state")

F64 = np.float64
D, RANK, N, TRUE_RANK = 97, 16, 200, 8


def _run(steps=12, seed=3):
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((D, TRUE_RANK)))[0].T
    pre = R.Pre(D, RANK)
    rows = []
    for _ in range(steps):
        X = R.low_rank_batch(rng, N, D, basis)
        before = pre.copy()
        out, g = pre.step(X)
        rows.append((X, out, g, before))
    return pre, rows, basis


def test_default_initial_state():
    pre = R.Pre(D, RANK)
    rt = pre.rt()
    assert np.allclose(rt @ rt.T, np.eye(RANK), atol=1e-14)
    assert np.count_nonzero(rt) == D and np.all(rt[np.arange(D) % RANK, np.arange(D)] > 0)
    assert pre.rho == pre.d[0] == F64(np.float32(1e-10)) and pre.t == 0
    # e = 1 / (1 + alpha + alpha R / D + 1) for d = rho
    assert np.allclose(pre.e(), 1.0 / (2.0 + 4.0 + 4.0 * RANK / D), rtol=1e-14)


def test_reference_after_12_steps():
    pre, rows, basis = _run()
    assert pre.t == 12
    rt = pre.rt()
    orth = np.linalg.norm(rt @ rt.T - np.eye(RANK))
    print(f"|R R^T - I|_F after 12 steps: {orth:.3e}")
    assert orth <= 1e-8
    for X, out, g, before in rows:
        trx = np.sum(X * X)
        rel = abs(np.sum(out * out) - trx) / trx
        assert rel <= 1e-10, rel
        assert g >= 1.0
    d = np.sort(pre.d)[::-1]
    print("d:", d)
    assert d[TRUE_RANK - 1] > 10.0 * d[TRUE_RANK]
    # the leading directions are the data's: the basis lies in the span of the top-8 rows of R_t
    top = rt[np.argsort(pre.d)[::-1][:TRUE_RANK]]
    assert np.linalg.norm(basis - basis @ top.T @ top) / np.linalg.norm(basis) < 0.05


def test_schedule_and_non_updating_steps():
    pre, rows, _ = _run(steps=14)
    # t = 10, 11 and 13 do not update; t = 12 does
    changed = [not np.array_equal(rows[i][3].W, rows[i + 1][3].W) for i in range(13)]
    assert changed == [True] * 10 + [False, False, True]


def test_gradient_form_equals_row_form():
    """preconditioning the rows of X_ext and dY and multiplying = the two rank-R corrections of G"""
    rng = np.random.default_rng(9)
    T, K, Nout = 64, 40, 24
    pin, pout = R.Pre(K + 1, 8), R.Pre(Nout, 8)
    X = np.hstack([rng.standard_normal((T, K)), np.ones((T, 1))])
    dY = rng.standard_normal((T, Nout))
    for _ in range(3):
        pin.step(X)
        pout.step(dY)
    a, b = pin.copy(), pout.copy()
    xh, gi = a.step(X)
    yh, go = b.step(dY)
    ref = xh.T @ yh
    got = R.precondition_gradient(X.T @ dY, gi, go, pin.proj(), pout.proj())
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-12


def test_operand_rows():
    x = np.arange(12, dtype=F64).reshape(6, 2)                  # 5 rows and a spare row 5
    m = R.operand_rows(x, 5, 5, (-1, 0), True)
    assert np.array_equal(m[:, 0], [0, 0, 2, 4, 6]) and np.array_equal(m[:, 2], [0, 2, 4, 6, 8])
    m = R.operand_rows(x, 5, 5, (0, 1), False, edges=[(1, 4, 5)])
    assert np.array_equal(m[:, 2], [2, 4, 6, 8, 10])
    m = R.operand_rows(x, 5, 5, (0, 1), False)
    assert np.array_equal(m[:, 2], [2, 4, 6, 8, 0])
