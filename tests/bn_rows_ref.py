"""Reference of training-mode BatchNorm on a row subset: the rule the row-subsampled
step follows, stated on full rows, beside tests/bn_train_ref.py and tests/bn_sites_ref.py (imported,
not edited).

The statistics of a governed BatchNorm run over a subset S of the rows (n = |S|); every row is
normalised by them. The backward is that forward's exact derivative: every row's output depends on
the statistics, so a and b sum over every row and divide by n; only the rows of S enter the
statistics, so only they take the correction term.

- bn_rows_forward / bn_rows_backward: the rule in numpy float64 (checked against torch float64
  autograd in test_bn_rows_ref.py). With S = every row they are bn_train_ref's.
- rows_rule(T): while it is entered, bn_train_ref.bn_train_forward / bn_train_backward follow the
  rule with S = {t : t = 0 (mod 3)} on every [T x D] tensor they are handed, and are themselves on
  anything else (a conv layer's [T H x F] view, a per-sequence BatchNorm's B rows).
- BnRowsOracle: BnTrainOracle or BnSitesOracle run under rows_rule: the staged network on full
  rows whose governed tdnnf and prefinal BatchNorms take their statistics from the rows 0 (mod 3).
  With the output gradient zero outside those rows it computes what the compact rows compute.
"""
import contextlib

import numpy as np

import bn_train_ref as br

EPS = br.EPS


def bn_rows_forward(r, S, eps=EPS, rms=1.0, drop=None, seg=None, x=None, bypass=0.0):
    """r [rows x D], S an index array of rows -> dict(mean, var, scale, shift, out): the statistics
    of r[S], out = (r scale + shift) drop[seg] + bypass x on every row."""
    r = np.asarray(r, np.float64)
    f = br.bn_train_forward(r[S], eps, rms)
    out = r * f["scale"] + f["shift"]
    if drop is not None:
        out = out * np.asarray(drop, np.float64)[np.asarray(seg)]
    if x is not None and bypass:
        out = out + bypass * np.asarray(x, np.float64)
    f["out"] = out
    return f


def bn_rows_backward(g, r, S, scale, shift, rms=1.0, drop=None, seg=None):
    """-> (a, b, gr): dy = g drop[seg], yhat = (r scale + shift) / rms, n = |S|,
    a = sum_all dy / n, b = sum_all dy yhat / n, gr = scale (dy - a - yhat b) on the rows of S and
    scale dy on the others: the gradient at r before the ReLU bit."""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    scale, shift = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    n = len(S)
    dy = g if drop is None else g * np.asarray(drop, np.float64)[np.asarray(seg)]
    yhat = (r * scale + shift) / rms
    a = dy.sum(0) / n
    b = (dy * yhat).sum(0) / n
    gr = scale * dy
    gr[S] = scale * (dy[S] - a - yhat[S] * b)
    return a, b, gr


def rows_mod3(T):
    return np.arange(0, T, 3)


@contextlib.contextmanager
def rows_rule(T):
    """bn_train_ref's two functions follow the row-subset rule on [T x D] tensors while entered"""
    S = rows_mod3(T)
    fwd0, bwd0 = br.bn_train_forward, br.bn_train_backward

    def fwd(r, eps=EPS, rms=1.0, drop=None, seg=None, x=None, bypass=0.0):
        if np.shape(r)[0] != T:
            return fwd0(r, eps, rms, drop, seg, x, bypass)
        return bn_rows_forward(r, S, eps, rms, drop, seg, x, bypass)

    def bwd(g, r, scale, shift, rms=1.0, drop=None, seg=None):
        if np.shape(r)[0] != T:
            return bwd0(g, r, scale, shift, rms, drop, seg)
        return bn_rows_backward(g, r, S, scale, shift, rms, drop, seg)

    br.bn_train_forward, br.bn_train_backward = fwd, bwd
    try:
        yield S
    finally:
        br.bn_train_forward, br.bn_train_backward = fwd0, bwd0


class BnRowsOracle:
    """inner: a BnTrainOracle or BnSitesOracle whose governed layers all lie in the row set (tdnnf
    and prefinal sites). forward / backward run it under rows_rule(T); everything else is the
    inner oracle's (acts, stats, act(), close())."""

    def __init__(self, inner):
        self.inner = inner

    def forward(self, features, **kw):
        with rows_rule(np.shape(features)[0]):
            return self.inner.forward(features, **kw)

    def backward(self, out_grad):
        with rows_rule(np.shape(out_grad)[0]):
            return self.inner.backward(out_grad)

    def relu_decisions(self):
        """layer -> the last forward's ReLU decisions (uint8, flat), the inner oracle's own"""
        if hasattr(self.inner, "masks") and not hasattr(self.inner, "r"):      # BnSitesOracle records them
            return {k: np.asarray(v).copy() for k, v in self.inner.masks.items()}
        out = {}
        for (lines, _gov, _byp), net in zip(self.inner.stages, self.inner.nets):  # BnTrainOracle: from its stages
            for line in lines:
                name = br._kv(line)["name"]
                m = net.mask(name)
                if m is not None:
                    out[name] = m
        return out

    def r_of(self, layer, which=0):
        """the tensor a governed BatchNorm normalised in the last forward, [T x D] float64"""
        if hasattr(self.inner, "r"):
            return np.asarray(self.inner.r[layer], np.float64)
        f = self.inner.fwd[layer]
        if "r" in f:
            return np.asarray(f["r"], np.float64)
        return np.asarray(f["r_small" if which else "r_big"], np.float64)

    def stats_of(self, layer, which=0):
        s = self.inner.stats
        return s[(layer, which)] if (layer, which) in s else s[layer]

    def __getattr__(self, name):
        return getattr(self.inner, name)
