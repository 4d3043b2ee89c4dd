"""tests/xent_ref.py (the float64 reference of kf_chain_xent) against torch's
float64 autograd, its ok = 0 rule, and the mutation check: a pdf map off by one, or the S term
dropped, lies beyond the bar tests/test_gpu_chain_xent.py holds the kernel to, on that test's
own cases. No GPU."""
import numpy as np
import pytest
import torch

import chain_ref as cr
import xent_ref as xr_


@pytest.mark.parametrize("T,P", [(7, 8), (50, 16)])
def test_against_autograd(T, P):
    """loss = -xr * w * sum post * log_softmax(z) with post constant: d loss / d z is the
    reference's gradient, and w * sum post * log_softmax(z) its objective, both at 1e-10."""
    xr, w = 0.1, 0.5
    rng = np.random.default_rng(T)
    f = cr.weighted_chain(3, min(T, 6), P)
    x = rng.standard_normal((T, P)) * 2.5
    total, post = cr.num_f64(f, x)
    assert np.isfinite(total) and post.sum() > 0
    z = torch.tensor(rng.standard_normal((T, P)) * 2.0, dtype=torch.float64, requires_grad=True)
    y = torch.log_softmax(z, dim=1)
    pt = torch.tensor(post, dtype=torch.float64)
    loss = -xr * w * (pt * y).sum()
    loss.backward()
    grad, objf, weight = xr_.xent_f64(f, x, y.detach().numpy(), xr, w)
    assert np.max(np.abs(grad - z.grad.numpy())) <= 1e-10
    assert abs(objf - w * float((pt * y).sum().detach())) <= 1e-10
    assert abs(objf * -xr - float(loss.detach())) <= 1e-10
    assert weight == w * T


def test_bad_sequence_is_all_zero():
    P, T = 13, 9
    f = cr.weighted_chain(5, 6, P)
    x = cr.outputs(1, T, P)
    y = xr_.xent_outputs(2, T, P)
    g, o, wt = xr_.xent_f64(f, x, y, 0.1, 1.0, ok=False)
    assert not np.any(g) and o == 0.0 and wt == T
    x[0, f["pdf1"][0] - 1] = np.inf                     # the numerator's total is not finite
    g, o, _ = xr_.xent_f64(f, x, y, 0.1, 1.0)
    assert not np.any(g) and o == 0.0
    c = xr_.case("p13_bad_zero")
    assert not np.any(c.ref(c.bad)[0]) and c.ref(c.bad)[1] == 0.0
    assert c.ref(1) == (c.ref(1)[0], 0.0, 0.0) and c.ref(1)[0].shape == (0, P)   # the zero-frame one
    assert np.any(c.ref(0)[0]) and c.ref(0)[1] < 0.0


@pytest.mark.parametrize("name", [n for n, c in xr_.CASES.items() if c["xr"] > 0])
def test_mutations_miss_the_gpu_bar(name):
    """Every live sequence of the GPU test's cases: the reference with the pdf map shifted by
    one column, and with the exp(y) * S term dropped, is more than the GPU test's gradient bar
    (chain_ref.grad_bar(ref, w * xr)) away from the reference; the shifted map also moves the
    objective per frame by more than 1e-3."""
    c = xr_.case(name)
    for i, T in enumerate(c.frames):
        if T == 0 or i == c.bad:
            continue
        ref, objf, _ = c.ref(i)
        bar = cr.grad_bar(ref, c.w * c.xr)
        for mut in (dict(shift=1), dict(with_s=False)):
            got, o2, _ = c.ref(i, **mut)
            share = float((np.abs(got - ref) / bar).max())
            print("%s seq %d %s: %.1f x the bar" % (name, i, mut, share))
            assert share > 1.0, (name, i, mut, share)
        assert abs(c.ref(i, shift=1)[1] - objf) / T > 1e-3
