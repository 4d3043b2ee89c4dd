"""The numpy reference of training-mode BatchNorm on a row subset (tests/bn_rows_ref.py, DESIGN.md
§28) against torch float64 autograd of "the statistics of r[S], applied to every row, times
target_rms, times a per-sequence dropout mask": 7 x 8 with S = the first 5 rows, 50 x 16 with S =
every third row. Bound 1e-10, test_bn_train_ref.py's (float64 on O(1) values, at most 50 rows)."""
import numpy as np
import pytest

import bn_rows_ref as rr
import bn_train_ref as br

BOUND = 1e-10

CASES = [(7, 8, np.arange(5)), (50, 16, np.arange(0, 50, 3))]


@pytest.mark.parametrize("n,D,S", CASES, ids=["7x8-first5", "50x16-mod3"])
@pytest.mark.parametrize("with_drop", [False, True])
def test_forward_backward_against_autograd(n, D, S, with_drop):
    import torch
    rng = np.random.default_rng(n * 100 + D + 7 * with_drop)
    eps, rms = 1e-3, 0.75
    r = np.maximum(rng.standard_normal((n, D)) + 0.3, 0.0)          # a ReLU output
    G = rng.standard_normal((n, D))
    seq = [0, n // 3, n // 2 + 1, n]
    seg = np.searchsorted(np.asarray(seq), np.arange(n), side="right") - 1
    drop = rng.uniform(0.4, 1.6, size=(3, D)) if with_drop else None

    f = rr.bn_rows_forward(r, S, eps, rms, drop, seg if with_drop else None)
    a, b, gr = rr.bn_rows_backward(G, r, S, f["scale"], f["shift"], rms, drop, seg if with_drop else None)

    rt = torch.tensor(r, dtype=torch.float64, requires_grad=True)
    St = torch.tensor(S, dtype=torch.long)
    mean = rt[St].mean(0)
    var = ((rt[St] - mean) ** 2).mean(0)
    y = (rt - mean) / torch.sqrt(var + eps) * rms
    if with_drop:
        y = y * torch.tensor(drop[seg], dtype=torch.float64)
    (y * torch.tensor(G, dtype=torch.float64)).sum().backward()

    assert np.abs(f["out"] - y.detach().numpy()).max() <= BOUND
    assert np.abs(f["mean"] - r[S].mean(0)).max() <= BOUND
    assert np.abs(f["var"] - r[S].var(0)).max() <= BOUND
    assert np.abs(gr - rt.grad.numpy()).max() <= BOUND
    # the rows outside S take no correction: scale dy alone
    out = np.setdiff1d(np.arange(n), S)
    dy = G * (drop[seg] if with_drop else 1.0)
    assert np.abs(gr[out] - f["scale"] * dy[out]).max() <= BOUND
    # a and b: sums over every row, divided by |S|
    yhat = (r - r[S].mean(0)) / np.sqrt(r[S].var(0) + eps)
    assert np.abs(a - dy.sum(0) / len(S)).max() <= BOUND and np.abs(b - (dy * yhat).sum(0) / len(S)).max() <= BOUND
    # and the all-rows rule's derivative is another one
    _, _, gr_all = br.bn_train_backward(G, r, f["scale"], f["shift"], rms, drop, seg if with_drop else None)
    assert np.abs(gr_all - rt.grad.numpy()).max() > 1e-3


def test_every_row_is_the_all_rows_rule():
    rng = np.random.default_rng(5)
    r, G = np.maximum(rng.standard_normal((11, 8)), 0.0), rng.standard_normal((11, 8))
    S = np.arange(11)
    f, f0 = rr.bn_rows_forward(r, S, 1e-3, 0.75), br.bn_train_forward(r, 1e-3, 0.75)
    for k in f0:
        assert np.array_equal(f[k], f0[k]), k
    got = rr.bn_rows_backward(G, r, S, f["scale"], f["shift"], 0.75)
    want = br.bn_train_backward(G, r, f0["scale"], f0["shift"], 0.75)
    for x, y in zip(got, want):
        assert np.abs(x - y).max() <= 1e-15


def test_rows_rule_patches_and_restores():
    """rows_rule swaps bn_train_ref's two functions for the rule on [T x D] tensors only, and puts
    them back"""
    rng = np.random.default_rng(6)
    T, D = 12, 8
    r, G = np.maximum(rng.standard_normal((T, D)), 0.0), rng.standard_normal((T, D))
    fwd0, bwd0 = br.bn_train_forward, br.bn_train_backward
    with rr.rows_rule(T) as S:
        assert np.array_equal(S, [0, 3, 6, 9])
        f = br.bn_train_forward(r, 1e-3, 1.0)
        assert np.abs(f["mean"] - r[S].mean(0)).max() <= 1e-15
        gr = br.bn_train_backward(G, r, f["scale"], f["shift"])[2]
        assert np.array_equal(gr[1], f["scale"] * G[1])
        other = br.bn_train_forward(r[:5], 1e-3, 1.0)              # not T rows: the all-rows rule
        assert np.abs(other["mean"] - r[:5].mean(0)).max() <= 1e-15
    assert br.bn_train_forward is fwd0 and br.bn_train_backward is bwd0


def test_policy_on_a_layout_only_net():
    """nnet_set_bn_train_rows needs no device: the default, the two policies, a bad value"""
    import kfp16
    from kfp16 import synth
    net = kfp16.Network(synth.load_xconfig("tiny.xconfig"), max_frames=64, layout_only=True)
    assert net.batchnorm_train_rows() == "all"
    net.set_batchnorm_train_rows("subsampled")
    assert net.batchnorm_train_rows() == "subsampled" and kfp16.nnet.nnet_bn_train_rows(net.h) == 1
    net.set_batchnorm_train_rows("all")
    assert net.batchnorm_train_rows() == "all"
    with pytest.raises(kfp16.KfError, match="unknown policy"):
        net.set_batchnorm_train_rows("some")
    assert kfp16.nnet.nnet_set_bn_train_rows(net.h, 2) == -1
    assert b"set_bn_train_rows" in kfp16.nnet.nnet_last_error()
    net.close()
