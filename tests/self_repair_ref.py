"""Reference of the ReLU unit statistics and self-repair: Kaldi's StoreStats and
RectifiedLinearComponent::RepairGradients on the sites training-mode BatchNorm governs, in numpy
float64 on top of tests/bn_train_ref.py and tests/bn_rows_ref.py (imported, not edited).

- relu_counts: deriv_sum's increment of one forward, per column or per block of a conv's view.
- repair_vector: the threshold rule. The comparisons are in double; the result is the fp32
  product fl32(k) fl32(S), negative for a dead unit: the gradients here are those of the loss
  nnet_sgd subtracts, so a negative term in dz raises the unit's bias.
- repair_backward: dz before its one fp16 rounding, scale (dy - a - yhat b) relu_bit + s on the
  statistics rows and scale dy relu_bit on the others: s is added where numpy turns g into the
  gradient at r, after the ReLU bit (a dead unit's bit is 0 on every row).
- sgd_step: the plain update, for the sign.
- SelfRepairOracle: the staged network reference (bn_sites_ref.BnSitesOracle) with the term in its
  backward; under bn_rows_ref.rows_rule it is the row-subsampled rule's.
- tdnnf_response: the gradients a tdnnf-layer's own parameters take from dz = 1 (x) s alone (a zero
  output gradient), with the clamped splices' edge rows, for the strided layers.
"""
import numpy as np

import bn_rows_ref as rr
import bn_sites_ref as bs
import bn_train_ref as br
from bn_sites_ref import _kv


def relu_counts(r, H=1):
    """r [rows x H F] -> #{r > 0} per block f = column h F + f (H = 1: per column), float64"""
    r = np.asarray(r)
    return (r.reshape(r.shape[0] * H, -1) > 0).sum(0).astype(np.float64)


def repair_vector(count, deriv_sum, k, lower=0.05, upper=0.95, S=1.0):
    """-> s float32 [D]"""
    d = np.asarray(deriv_sum, np.float64)
    ks = np.float32(np.float32(k) * np.float32(S))
    s = np.zeros(d.shape, np.float32)
    if float(count) == 0.0:
        return s
    s[d <= np.float64(lower) * np.float64(count)] = -ks
    s[d > np.float64(upper) * np.float64(count)] = ks
    return s


def repair_backward(g, r, scale, shift, rms, bits, s, stat_rows=None, drop=None, seg=None):
    """-> (a, b, dz) in float64, dz before its rounding to fp16. stat_rows None: every row."""
    rows = np.asarray(r).shape[0]
    n = rows if stat_rows is None else int(stat_rows)
    if n == rows:
        a, b, gr = br.bn_train_backward(g, r, scale, shift, rms, drop, seg)
    else:
        a, b, gr = rr.bn_rows_backward(g, r, np.arange(n), scale, shift, rms, drop, seg)
    dz = gr * np.asarray(bits, np.float64)
    dz[:n] += np.asarray(s, np.float64)
    return a, b, dz


def sgd_step(param, grad, lr):
    return np.asarray(param, np.float64) - lr * np.asarray(grad, np.float64)


def tdnnf_response(x, W1, W2, s, stride):
    """A tdnnf-layer with time stride `stride` > 0 whose dz is s on every row: x [T x din] its input,
    W1 [2 din x bn] and W2 [2 bn x dout] as the product stores them. Forward: bott(t) = [x(t -
    stride) | x(t)] W1 and the affine reads [bott(t) | bott(t + stride)], both clamped to the
    tensor's rows. -> dict(LinearW, AffineW, AffineBias) in float64."""
    x, W1, W2 = (np.asarray(v, np.float64) for v in (x, W1, W2))
    T, bn = x.shape[0], W1.shape[1]
    t = np.arange(T)
    lo, hi = np.maximum(t - stride, 0), np.minimum(t + stride, T - 1)
    X = np.concatenate([x[lo], x], 1)
    bott = (X @ W1).astype(np.float16).astype(np.float64)
    A = np.concatenate([bott, bott[hi]], 1)
    dz = np.tile(np.asarray(s, np.float64).astype(np.float16).astype(np.float64), (T, 1))
    dbott = dz @ W2[:bn].T
    np.add.at(dbott, hi, dz @ W2[bn:].T)  # (the clamped rows pile up on row T - 1)
    return {"LinearW": X.T @ dbott, "AffineW": A.T @ dz, "AffineBias": dz.sum(0)}


class SelfRepairOracle(bs.BnSitesOracle):
    """BnSitesOracle (imported, not edited) whose backward adds the repair term where numpy turns g
    into the gradient at r: dz = (gradient at r) relu_bit + s on the statistics rows.

    repair: layer -> s [D] (float32, fl32(k) signed). rows: None, or the index array of the
    statistics rows of the [T x D] sites (the row-subsampled rule, run under bn_rows_ref.rows_rule);
    a conv site's statistics always run over every row.

    A governed conv or tdnnf stage's oracle applies the layer's ReLU bit to whatever it is handed,
    which would drop the term of an element whose bit is 0. So for the columns with a term numpy
    applies the bit itself and adds s, and the stage is forwarded again with those columns' ReLU
    decisions forced to 1 before its backward: the oracle's bit is then the identity there. Nothing
    the backward reads depends on those decisions but the bit (the layer is the stage's last; its
    weight, bias and input gradients read the mask, the bottleneck or the input). A governed
    prefinal-layer is a numpy stage: bn_sites_ref.prefinal_backward restated with the term."""

    def __init__(self, *args, repair=None, rows=None, **kw):
        super().__init__(*args, **kw)
        self.repair, self.rows = dict(repair or {}), rows

    def _term(self, gov, n, H):
        """(columns with a term, s, the statistics rows of the [n H x F] view) or None"""
        s = self.repair.get(gov)
        if s is None or not np.any(s):
            return None
        sel = np.arange(n * H) if (H > 1 or self.rows is None) else np.asarray(self.rows)
        return np.nonzero(s)[0], np.asarray(s, np.float64), sel

    def backward(self, out_grad):
        g = np.ascontiguousarray(out_grad, np.float32)
        grads = {}
        for si in range(len(self.stages) - 1, -1, -1):
            kind, lines, gov, gkind = self.stages[si]
            x, net = self.stage_in[si], self.nets[si]
            if kind == "prefinal":
                xx, W, W2, mask, aux, c0, c1 = self.fwd[gov]["cache"]
                dz_small = bs.f16(bs._bn_back(g.astype(np.float64), c1))
                g_big = bs.f16(dz_small @ W2.T)
                w = bs._bn_back(g_big, c0) * mask
                t = self._term(gov, w.shape[0], 1)
                if t is not None:
                    cols, s, sel = t
                    w[np.ix_(sel, cols)] += s[cols]
                dz_big = bs.f16(w)
                grads[gov + ".BigW"], grads[gov + ".BigBias"], grads[gov + ".SmallW"] = xx.T @ dz_big, dz_big.sum(0).reshape(1, -1), aux.T @ dz_small
                g = bs.f16(dz_big @ W.T).astype(np.float32)
                continue
            gtop = g
            if gov is not None:
                f = self.fwd[gov]
                H, F = f["H"], f["F"]
                gr = bs.bn_block_backward(g, f["r"], H, F, f["scale"], f["shift"])[2]
                t = self._term(gov, gr.shape[0], H)
                if t is not None:
                    cols, s, sel = t
                    bits = np.asarray(self.masks[gov]).reshape(-1, F)
                    g2 = gr.reshape(-1, F).copy()
                    g2[:, cols] *= bits[:, cols]
                    g2[np.ix_(sel, cols)] += s[cols]
                    forced = bits.copy()
                    forced[:, cols] = 1
                    names = [_kv(l)["name"] for l in lines]
                    fm = {n: self.masks[n] for n in names if n in self.masks}
                    fm[gov] = np.ascontiguousarray(forced.reshape(-1), np.uint8)
                    if si == 0 and self.ivec is not None:
                        net.forward(x, force_masks=fm, ivectors=np.asarray(self.ivec, np.float32), seq_off=self.seq_off)
                    else:
                        net.forward(x, force_masks=fm)
                    gr = g2.reshape(gr.shape)
                gtop = gr.astype(np.float32)
            net.backward(gtop)
            for k, v in net.grads().items():
                if not k.startswith("stage-in."):
                    grads[k] = v
            if si == 0:
                self._ivector_gradient(net, grads)
            else:
                d = x.shape[1]
                gin = np.ctypeslib.as_array(net.net.gact[0], shape=(x.shape[0] * d,)).reshape(-1, d).astype(np.float64)
                if gov is not None and self.fwd[gov]["bypass"] > 0:
                    gin = gin + self.fwd[gov]["bypass"] * g.astype(np.float64)
                g = gin.astype(np.float32)
        return grads
