"""The numpy reference of the training-mode BatchNorm (tests/bn_train_ref.py) against torch float64
autograd: torch.nn.functional.batch_norm(training=True) times target_rms, a per-sequence dropout
mask and a bypass. Bound 1e-10 (float64 on O(1) values: both sides carry a few 1e-16 per
operation over at most 50 rows)."""
import numpy as np
import pytest

import bn_train_ref as br

BOUND = 1e-10


@pytest.mark.parametrize("n,D", [(7, 8), (50, 16)])
@pytest.mark.parametrize("with_drop", [False, True])
@pytest.mark.parametrize("bypass", [0.0, 0.66])
def test_forward_backward_against_autograd(n, D, with_drop, bypass):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(n * 100 + D + 7 * with_drop)
    eps, rms = 1e-3, 0.75
    r = np.maximum(rng.standard_normal((n, D)) + 0.3, 0.0)          # a ReLU output
    x = rng.standard_normal((n, D))
    G = rng.standard_normal((n, D))
    seq = [0, n // 3, n // 2 + 1, n]
    seg = np.searchsorted(np.asarray(seq), np.arange(n), side="right") - 1
    drop = rng.uniform(0.4, 1.6, size=(3, D)) if with_drop else None

    f = br.bn_train_forward(r, eps, rms, drop, seg if with_drop else None, x, bypass)
    a, b, gr = br.bn_train_backward(G, r, f["scale"], f["shift"], rms, drop, seg if with_drop else None)

    rt = torch.tensor(r, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    y = F.batch_norm(rt, None, None, training=True, eps=eps) * rms
    if with_drop:
        y = y * torch.tensor(drop[seg], dtype=torch.float64)
    y = y + bypass * xt
    (y * torch.tensor(G, dtype=torch.float64)).sum().backward()

    assert np.abs(f["out"] - y.detach().numpy()).max() <= BOUND
    assert np.abs(f["mean"] - r.mean(0)).max() <= BOUND
    assert np.abs(f["var"] - r.var(0)).max() <= BOUND                # the biased variance
    assert np.abs(gr - rt.grad.numpy()).max() <= BOUND
    assert np.abs(bypass * G - xt.grad.numpy()).max() <= BOUND       # the bypass gradient is unchanged
    # a and b are what they are named: the column means of dy and of dy yhat
    dy = G * (drop[seg] if with_drop else 1.0)
    yhat = (r - r.mean(0)) / np.sqrt(r.var(0) + eps)
    assert np.abs(a - dy.mean(0)).max() <= BOUND and np.abs(b - (dy * yhat).mean(0)).max() <= BOUND


def test_constant_and_zero_columns():
    """var is floored at 0, and a constant column maps to exactly shift + r scale = 0"""
    r = np.zeros((9, 8))
    r[:, 1] = 2.5
    r[:, 2] = np.arange(9)
    f = br.bn_train_forward(r, 1e-3, 1.0)
    assert np.all(f["var"][:2] == 0.0) and f["var"][2] > 0
    assert np.abs(f["out"][:, :2]).max() <= 1e-12
    assert abs(f["scale"][0] - 1.0 / np.sqrt(1e-3)) <= 1e-12
