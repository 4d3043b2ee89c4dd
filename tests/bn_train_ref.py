"""Reference of the TDNN-F training-mode BatchNorm: Kaldi's BatchNormComponent in
training mode, on r = rne_fp16(relu(affine + bias)).

- bn_train_forward / bn_train_backward: the rule of kf_ops.h kf_bn_train_* in numpy float64
  (checked against torch float64 autograd in test_bn_train_ref.py).
- BnTrainOracle: forward / backward of a network whose governed tdnnf-layers normalise by their
  batch statistics, built from the committed CPU oracle (oracle/oracle.py OracleNet, imported, not
  edited) run in stages. A governed tdnnf-layer is a stage of its own with bypass-scale=0 and an
  identity BatchNorm, so the oracle yields r; BatchNorm, dropout and bypass are applied here in
  float64. In the backward numpy turns g into the gradient at r, the stage's oracle backward
  takes it from there (it applies the ReLU bit and its fp16 rounding of dz), and bypass * g is
  added to the stage's input gradient.

Its own error against the rule: a stage hands down the fp16-rounded input gradient plus the
float64 bypass term where the product's epilogue rounds their sum once (2^-11 relative per
layer), far below the 2e-3 / 5e-3 bounds the comparisons use.
"""
import numpy as np

EPS = 1e-3  # the oracle's BatchNorm epsilon (oracle.py OracleNet._bn) and synth.init_network's


def bn_train_forward(r, eps=EPS, rms=1.0, drop=None, seg=None, x=None, bypass=0.0):
    """r [n x D] -> dict(mean, var, scale, shift, out) in float64:
    mean = sum r / n, var = max(0, sum r^2 / n - mean^2), scale = rms (var + eps)^-1/2,
    shift = -mean scale, out = (r scale + shift) drop[seg] + bypass x."""
    r = np.asarray(r, np.float64)
    n = r.shape[0]
    mean = r.sum(0) / n
    var = np.maximum((r * r).sum(0) / n - mean * mean, 0.0)
    scale = rms / np.sqrt(var + eps)
    shift = -mean * scale
    out = r * scale + shift
    if drop is not None:
        out = out * np.asarray(drop, np.float64)[np.asarray(seg)]
    if x is not None and bypass:
        out = out + bypass * np.asarray(x, np.float64)
    return dict(mean=mean, var=var, scale=scale, shift=shift, out=out)


def bn_train_backward(g, r, scale, shift, rms=1.0, drop=None, seg=None):
    """-> (a, b, gr): dy = g drop[seg], yhat = (r scale + shift) / rms, a = sum dy / n,
    b = sum dy yhat / n, gr = scale (dy - a - yhat b): the gradient at r before the ReLU bit."""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    scale, shift = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    n = r.shape[0]
    dy = g if drop is None else g * np.asarray(drop, np.float64)[np.asarray(seg)]
    yhat = (r * scale + shift) / rms
    a = dy.sum(0) / n
    b = (dy * yhat).sum(0) / n
    return a, b, scale * (dy - a - yhat * b)


def _kv(line):
    return dict(t.split("=", 1) for t in line.split()[1:] if "=" in t)


class BnTrainOracle:
    """The oracle's network with training-mode BatchNorm on the `governed` tdnnf-layers.

    masks: layer -> dropout mask [B x dim] (with seq_row0, the sequences' first rows and T), or
    None. After forward(): acts, stats[layer] = (mean, var) and r[layer]."""

    def __init__(self, xconfig: str, params: dict, bns: dict, governed, masks=None, seq_row0=None, rms=1.0, threads=8):
        import oracle
        self.oracle = oracle
        self.params, self.bns, self.masks = params, bns, masks or {}
        self.seq = None if seq_row0 is None else np.asarray(seq_row0, np.int64)
        self.rms, self.threads = float(rms), threads
        # var + eps == 1 exactly in fp32: the stage's BatchNorm is the identity, bit for bit
        self.var1 = np.float32(0.999)
        assert np.float32(self.var1 + np.float32(EPS)) == np.float32(1.0)
        inputs, lines = [], []
        for raw in xconfig.splitlines():
            line = raw.strip()
            if not line or line.startswith("#"):
                continue
            (inputs if line.split()[0] == "input" else lines).append(line)
        assert len(inputs) == 1, "one input"
        self.first_input = inputs[0]
        self.stages, cur = [], []
        for line in lines:
            kv = _kv(line)
            if kv["name"] in governed:
                assert line.split()[0] == "tdnnf-layer"
                if cur:
                    self.stages.append((cur, None, 0.0))
                byp = float(kv.get("bypass-scale", 0.66))
                toks = [t for t in line.split() if not t.startswith("bypass-scale=")] + ["bypass-scale=0"]
                self.stages.append(([" ".join(toks)], kv["name"], byp))
                cur = []
            else:
                cur.append(line)
        if cur:
            self.stages.append((cur, None, 0.0))
        assert sum(1 for s in self.stages if s[1]) == len(set(governed))
        self.acts, self.stats, self.r, self.fwd = {}, {}, {}, {}
        self.stage_in, self.nets = [], []

    def _net(self, si, din):
        lines, gov, _ = self.stages[si]
        params, bns = dict(self.params), dict(self.bns)
        if si == 0:
            text = "\n".join([self.first_input] + lines) + "\n"
        else:
            text = "\n".join([f"input name=input dim={din}", f"linear-component name=stage-in dim={din}"] + lines) + "\n"
            params["stage-in.W"] = np.eye(din, dtype=np.float32)
        if gov:
            d = self.params[gov + ".AffineBias"].size
            bns[(gov, 0)] = (np.zeros(d, np.float32), np.full(d, self.var1, np.float32), np.ones(d, np.float32),
                             np.zeros(d, np.float32))
        return self.oracle.OracleNet(text, params, bns, round_mode=self.oracle.ROUND_FUSED, threads=self.threads)

    def _seg(self, T):
        return None if self.seq is None else (np.searchsorted(self.seq, np.arange(T), side="right") - 1)

    def forward(self, features, force_masks=None):
        x = np.ascontiguousarray(features, np.float32)
        T = x.shape[0]
        self.close()
        self.stage_in = []
        for si, (lines, gov, byp) in enumerate(self.stages):
            self.stage_in.append(x)
            names = [_kv(l)["name"] for l in lines]
            fm = {n: force_masks[n] for n in names if force_masks and n in force_masks} or None
            net = self._net(si, x.shape[1])
            net.forward(x, force_masks=fm)
            self.nets.append(net)
            if gov is None:
                for n in names:
                    self.acts[n] = net.act(n)
                x = net.act(names[-1])
                continue
            r = net.act(gov)
            self.r[gov] = r
            drop = self.masks.get(gov)
            bypass = byp if (byp > 0 and x.shape[1] == r.shape[1]) else 0.0
            f = bn_train_forward(r, EPS, self.rms, drop, self._seg(T) if drop is not None else None, x, bypass)
            self.fwd[gov] = f
            self.stats[gov] = (f["mean"], f["var"])
            x = f["out"].astype(np.float16).astype(np.float32)  # the layer's activation is fp16
            self.acts[gov] = x
        return x

    def act(self, name):
        return self.acts[name]

    def backward(self, out_grad):
        """-> gradients keyed by the product's parameter names"""
        g = np.ascontiguousarray(out_grad, np.float32)
        grads = {}
        for si in range(len(self.stages) - 1, -1, -1):
            lines, gov, byp = self.stages[si]
            x, net = self.stage_in[si], self.nets[si]
            gtop = g
            if gov is not None:
                f, drop = self.fwd[gov], self.masks.get(gov)
                _, _, gr = bn_train_backward(g, self.r[gov], f["scale"], f["shift"], self.rms, drop,
                                             self._seg(x.shape[0]) if drop is not None else None)
                gtop = gr.astype(np.float32)
            net.backward(gtop)
            for k, v in net.grads().items():
                if not k.startswith("stage-in."):
                    grads[k] = v
            if si > 0:
                d = x.shape[1]
                gin = np.ctypeslib.as_array(net.net.gact[0], shape=(x.shape[0] * d,)).reshape(-1, d).astype(np.float64)
                if gov is not None and byp > 0 and d == g.shape[1]:
                    gin = gin + byp * g.astype(np.float64)
                g = gin.astype(np.float32)
        return grads

    def close(self):
        for net in self.nets:
            net.close()
        self.nets = []
