"""Reference of the training-mode BatchNorm on the conv, prefinal and batchnorm-component sites
(DESIGN.md §27), beside tests/bn_train_ref.py (imported, not edited) for the TDNN-F layers.

- bn_block_forward / bn_block_backward: the rule of kf_ops.h kf_bn_block_* in numpy float64. A
  BatchNorm with block-dim F on r [rows x H F] is the column rule of bn_train_ref on the dense
  [rows H x F] view (checked against torch float64 autograd in test_bn_sites_ref.py).
- prefinal_forward / prefinal_backward: a prefinal-layer in numpy float64 with the product's fp16
  rounding points (r_big, aux, r_small, act; dz_small, g_big, dz_big, the input gradient), each
  BatchNorm frozen or in training mode. The frozen form is checked against the committed oracle.
- component_stats / ivector_branch_backward: a batchnorm-component in training mode. Its forward
  is the frozen forward fed the batch statistics, so the oracle computes it; its backward exists
  only on the per-sequence branch (ivector-batchnorm above ivector-linear) and is restated here.
- BnSitesOracle: a network with any set of sites governed, built from the committed CPU oracle
  run in stages, on BnTrainOracle's pattern: a governed conv or tdnnf layer ends a stage whose
  oracle BatchNorm is the identity, so the oracle yields r and numpy normalises it; a governed
  prefinal-layer is a numpy stage of its own; a governed batchnorm-component stays inside its
  stage as a frozen BatchNorm fed the batch statistics.

The reference's own error against the rule is BnTrainOracle's: a stage hands down the
fp16-rounded input gradient where the product rounds once more or less (2^-11 relative per
stage), far below the 2e-3 / 5e-3 bounds of the comparisons.
"""
import numpy as np

import bn_train_ref as br

EPS = br.EPS
SITE_KINDS = {"tdnnf": "tdnnf-layer", "conv": "conv-relu-batchnorm-layer", "prefinal": "prefinal-layer",
              "batchnorm": "batchnorm-component"}


def f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


# ---------------------------------------------------------------------------
# the block rule
# ---------------------------------------------------------------------------
def bn_block_forward(r, H, F, eps=EPS, rms=1.0):
    """r [rows x H F], column h F + f in block f -> dict(mean, var, scale, shift [F], out)"""
    r = np.asarray(r, np.float64)
    rows = r.shape[0]
    assert r.shape[1] == H * F
    f = br.bn_train_forward(r.reshape(rows * H, F), eps, rms)
    f["out"] = f["out"].reshape(rows, H * F)
    return f


def bn_block_backward(g, r, H, F, scale, shift, rms=1.0, mask=None):
    """-> (a, b [F], gr [rows x H F]): gr = scale (g - a - yhat b) relu_bit (mask None: 1)"""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    rows = r.shape[0]
    a, b, gr = br.bn_train_backward(g.reshape(rows * H, F), r.reshape(rows * H, F), scale, shift, rms)
    gr = gr.reshape(rows, H * F)
    if mask is not None:
        gr = gr * np.asarray(mask, np.float64).reshape(rows, H * F)
    return a, b, gr


# ---------------------------------------------------------------------------
# a BatchNorm, frozen or in training mode, as the numpy stages use it
# ---------------------------------------------------------------------------
def _bn(r, spec, rms):
    """spec None: training mode; else the frozen (mean, var, gamma, beta). -> (out, cache)"""
    if spec is None:
        f = br.bn_train_forward(r, EPS, rms)
        return f["out"], dict(train=True, r=r, scale=f["scale"], shift=f["shift"], rms=rms, stats=(f["mean"], f["var"]))
    m, v, ga, be = (np.asarray(t, np.float64) for t in spec)
    scale = ga * rms / np.sqrt(v + EPS)
    return r * scale + (be - m * scale), dict(train=False, scale=scale)


def _bn_back(g, c):
    if not c["train"]:
        return g * c["scale"]
    return br.bn_train_backward(g, c["r"], c["scale"], c["shift"], c["rms"])[2]


def prefinal_forward(x, W, b, W2, bn0=None, bn1=None, force_mask=None):
    """x [T x din] fp16 values; W [din x big], b [big], W2 [big x small]; bn0 / bn1 None: training
    mode, else the frozen (mean, var, gamma, beta). force_mask [T x big]: ReLU decisions to replay.
    -> dict(act, aux, r_big, r_small, mask, stats0, stats1, cache)"""
    x, W, W2 = (np.asarray(t, np.float64) for t in (x, W, W2))
    z = x @ W + np.asarray(b, np.float64).reshape(1, -1)
    mask = (z > 0) if force_mask is None else np.asarray(force_mask).reshape(z.shape).astype(bool)
    r_big = f16(np.where(mask, z, 0.0))
    y0, c0 = _bn(r_big, bn0, 1.0)
    aux = f16(y0)
    r_small = f16(aux @ W2)
    y1, c1 = _bn(r_small, bn1, 1.0)
    act = f16(y1)
    return dict(act=act, aux=aux, r_big=r_big, r_small=r_small, mask=mask, stats0=c0.get("stats"), stats1=c1.get("stats"),
                cache=(x, W, W2, mask, aux, c0, c1))


def prefinal_backward(g, fwd):
    """g [T x small]: the stored (fp16) gradient at the layer's output. -> (gW, gb, gW2, gin)"""
    x, W, W2, mask, aux, c0, c1 = fwd["cache"]
    dz_small = f16(_bn_back(np.asarray(g, np.float64), c1))
    gW2 = aux.T @ dz_small
    g_big = dz_small @ W2.T
    if c0["train"]:
        g_big = f16(g_big)                       # the raw gradient is a tensor of its own there
    dz_big = f16(_bn_back(g_big, c0) * mask)
    return x.T @ dz_big, dz_big.sum(0), gW2, f16(dz_big @ W.T)


# ---------------------------------------------------------------------------
# batchnorm-component
# ---------------------------------------------------------------------------
def component_stats(r, rms):
    """the batch statistics of a batchnorm-component's input r [rows x D]: (mean, var), and its
    output in fp16 values"""
    f = br.bn_train_forward(r, EPS, rms)
    return (f["mean"], f["var"]), f16(f["out"])


def ivector_branch_backward(g_combine, seq_off, height, nf1, nf2, r, rms, ivec, train=True, frozen=None):
    """The gradient of ivector-linear's weight through a per-sequence batchnorm-component.
    g_combine [T x height (nf1 + nf2)]: the stored gradient at combine-feature-maps' output;
    r [B x D] = rne_fp16(ivec W), the component's input. frozen: (mean, var) when not train."""
    g = np.asarray(g_combine, np.float64)
    B, nf = len(seq_off) - 1, nf1 + nf2
    db = np.zeros((B, height * nf2))
    for s in range(B):
        blk = g[seq_off[s]:seq_off[s + 1]].reshape(-1, height, nf)[:, :, nf1:]
        db[s] = blk.sum(0).reshape(-1)
    db = f16(db)
    if train:
        f = br.bn_train_forward(r, EPS, rms)
        dz = br.bn_train_backward(db, r, f["scale"], f["shift"], rms)[2]
    else:
        dz = db * (rms / np.sqrt(np.asarray(frozen[1], np.float64) + EPS))
    return np.asarray(ivec, np.float64).T @ f16(dz)


# ---------------------------------------------------------------------------
# the staged network
# ---------------------------------------------------------------------------
def matched_bns(xconfig, params, bns, features, sites, ivectors=None, seq_off=None, threads=8):
    """The frozen statistics of a network comparison with `sites` governed. The layers that stay
    frozen get statistics that match the data, as a trained model's do: those the BatchNorm sees on
    `features` with all sites in training mode (gamma 1, beta 0). synth.init_network's are drawn at
    random; under them a quarter of tiny.xconfig's prefinal ReLU columns have a variance below
    4 eps, and a governed BatchNorm above layers frozen at them amplifies the fp16 differences
    between two correct evaluations of the network 3.6 times (BnSitesOracle.amplification), which
    says nothing about either. The governed BatchNorms keep init_network's random statistics: they
    never enter the train-mode computation, and a forward that applied them in place of the batch
    statistics lies far from the reference (asserted in test_bn_sites_ref.py). With every site
    governed, or only the batchnorm-components (nothing lies below them), nothing is replaced."""
    kinds = {SITE_KINDS[s] for s in sites}
    if kinds == {SITE_KINDS["batchnorm"]} or kinds == set(SITE_KINDS.values()):
        return dict(bns)
    ref = BnSitesOracle(xconfig, params, bns, list(SITE_KINDS), threads=threads)
    ref.forward(features, ivectors=ivectors, seq_off=seq_off)
    out = dict(bns)
    for (name, which), (m, v) in ref.stats.items():
        if ref.layer_line[name].split()[0] in kinds:
            continue
        d = m.size
        out[(name, which)] = (m.astype(np.float32), v.astype(np.float32), np.ones(d, np.float32), np.zeros(d, np.float32))
    ref.close()
    return out


def _kv(line):
    return dict(t.split("=", 1) for t in line.split()[1:] if "=" in t)


class BnSitesOracle:
    """The oracle's network with training-mode BatchNorm on the sites named (SITE_KINDS' keys).

    After forward(): acts[layer], stats[(layer, which)] = (mean, var), masks[layer] (uint8 ReLU
    decisions, flat). backward() -> gradients keyed by the product's parameter names."""

    def __init__(self, xconfig, params, bns, sites, threads=8):
        import oracle
        self.oracle = oracle
        self.params, self.bns, self.threads = params, dict(bns), threads
        self.kinds = {SITE_KINDS[s] for s in sites}
        self.var1 = np.float32(0.999)       # var + eps == 1 exactly in fp32: an identity BatchNorm
        assert np.float32(self.var1 + np.float32(EPS)) == np.float32(1.0)
        self.inputs, self.lines = [], []
        for raw in xconfig.splitlines():
            line = raw.strip()
            if line and not line.startswith("#"):
                (self.inputs if line.split()[0] == "input" else self.lines).append(line)
        # stages: ("oracle", lines, governed layer or None, its kind) | ("prefinal", [line], name, kind)
        self.stages, cur = [], []
        self.components = []                # governed batchnorm-components (name, line)
        for line in self.lines:
            kind, kv = line.split()[0], _kv(line)
            gov = kind in self.kinds
            if gov and kind == "batchnorm-component":
                self.components.append((kv["name"], line))
                gov = False
            if gov and kind == "prefinal-layer":
                if cur:
                    self.stages.append(("oracle", cur, None, None))
                self.stages.append(("prefinal", [line], kv["name"], kind))
                cur = []
            elif gov:
                toks = line.split()
                if kind == "tdnnf-layer":   # (the bypass is added here, as in BnTrainOracle)
                    toks = [t for t in toks if not t.startswith("bypass-scale=")] + ["bypass-scale=0"]
                self.stages.append(("oracle", cur + [" ".join(toks)], kv["name"], kind))
                cur = []
            else:
                cur.append(line)
        if cur:
            self.stages.append(("oracle", cur, None, None))
        self.layer_line = {_kv(l)["name"]: l for l in self.lines}
        self.acts, self.stats, self.masks, self.fwd = {}, {}, {}, {}
        self.stage_in, self.stage_out, self.nets = [], [], []

    # -- governed batchnorm-components: the batch statistics of their input, fed as frozen ones
    def _component_inputs(self, features, ivectors):
        out = {}
        prev = None
        for line in self.lines:
            kind, kv = line.split()[0], _kv(line)
            name = kv["name"]
            if (name, line) in self.components:
                src = kv.get("input", prev)
                sk = self.layer_line[src].split()[0]
                rms = float(kv.get("target-rms", 1.0))
                if sk == "idct-layer":
                    text = "\n".join([l for l in self.inputs if _kv(l)["name"] == _kv(self.layer_line[src]).get("input", "input")]
                                     + [self.layer_line[src]]) + "\n"
                    net = self.oracle.OracleNet(text, self.params, {}, round_mode=self.oracle.ROUND_FUSED, threads=self.threads)
                    net.forward(features)
                    r = net.act(src).astype(np.float64)
                    net.close()
                else:
                    assert sk == "linear-component" and "ReplaceIndex" in self.layer_line[src], "per-sequence linear-component"
                    r = f16(np.asarray(ivectors, np.float64) @ np.asarray(self.params[src + ".W"], np.float64))
                out[name] = (r, rms, src)
            prev = name
        return out

    def _net(self, si, din):
        kind, lines, gov, gkind = self.stages[si]
        params, bns = dict(self.params), dict(self.bns)
        if si == 0:
            text = "\n".join(self.inputs + lines) + "\n"
        else:
            text = "\n".join([f"input name=input dim={din}", f"linear-component name=stage-in dim={din}"] + lines) + "\n"
            params["stage-in.W"] = np.eye(din, dtype=np.float32)
        if gov:
            d = self._bn_len(gov, gkind)
            bns[(gov, 0)] = (np.zeros(d, np.float32), np.full(d, self.var1, np.float32), np.ones(d, np.float32),
                             np.zeros(d, np.float32))
        return self.oracle.OracleNet(text, params, bns, round_mode=self.oracle.ROUND_FUSED, threads=self.threads)

    def _bn_len(self, name, kind):
        kv = _kv(self.layer_line[name])
        return int(kv["num-filters-out"]) if kind == "conv-relu-batchnorm-layer" else int(kv["dim"])

    def forward(self, features, force_masks=None, ivectors=None, seq_off=None):
        x = np.ascontiguousarray(features, np.float32)
        self.close()
        self.stage_in, self.stage_out, self.ivec, self.seq_off = [], [], ivectors, seq_off
        self.comp_in = self._component_inputs(x, ivectors)
        for name, (r, rms, _) in self.comp_in.items():
            (m, v), _out = component_stats(r, rms)
            self.stats[(name, 0)] = (m, v)
            d = m.size
            self.bns[(name, 0)] = (m.astype(np.float32), v.astype(np.float32), np.ones(d, np.float32), np.zeros(d, np.float32))
        for si in range(len(self.stages)):
            self.stage_in.append(x)
            x, net = self._stage_forward(si, x, force_masks, True)
            self.nets.append(net)
            self.stage_out.append(x)
        return x

    def _stage_forward(self, si, x, force_masks, record):
        """stage si on input x -> (its output in fp16 values, its oracle net or None); record: keep
        the activations, statistics, masks and what the backward needs"""
        kind, lines, gov, gkind = self.stages[si]
        if kind == "prefinal":
            p = self.params
            fm = force_masks.get(gov) if force_masks else None
            f = prefinal_forward(x, p[gov + ".BigW"], np.asarray(p[gov + ".BigBias"]).reshape(-1), p[gov + ".SmallW"],
                                 force_mask=fm)
            out = f["act"].astype(np.float32)
            if record:
                self.fwd[gov] = f
                self.stats[(gov, 0)], self.stats[(gov, 1)] = f["stats0"], f["stats1"]
                self.masks[gov] = f["mask"].astype(np.uint8).reshape(-1)
                self.acts[gov] = out
            return out, None
        names = [_kv(l)["name"] for l in lines]
        fm = {n: force_masks[n] for n in names if force_masks and n in force_masks} or None
        net = self._net(si, x.shape[1])
        if si == 0 and self.ivec is not None:
            net.forward(x, force_masks=fm, ivectors=np.asarray(self.ivec, np.float32), seq_off=self.seq_off)
        else:
            net.forward(x, force_masks=fm)
        if record:
            for n in names:
                m = net.mask(n)
                if m is not None:
                    self.masks[n] = m
            for n in names[:-1] if gov else names:
                self.acts[n] = net.act(n)
        if gov is None:
            return net.act(names[-1]), net
        r = net.act(gov).astype(np.float64)
        kv = _kv(self.layer_line[gov])
        if gkind == "conv-relu-batchnorm-layer":
            F = int(kv["num-filters-out"])
            H = r.shape[1] // F
            f = bn_block_forward(r, H, F)
            f["H"], f["F"], f["bypass"] = H, F, 0.0
        else:
            byp = float(kv.get("bypass-scale", 0.66))
            byp = byp if (byp > 0 and x.shape[1] == r.shape[1]) else 0.0
            f = br.bn_train_forward(r, EPS, 1.0, None, None, x, byp)
            f["H"], f["F"], f["bypass"] = 1, r.shape[1], byp
        f["r"] = r
        out = f["out"].astype(np.float16).astype(np.float32)
        if record:
            self.fwd[gov] = f
            self.stats[(gov, 0)] = (f["mean"], f["var"])
            self.acts[gov] = out
        return out, net

    def amplification(self, delta=1e-3, seed=0):
        """How much each governed stage amplifies an error of its input: the stage again on its
        input plus noise of delta x the input's rms, the relative Frobenius change of its output
        over that of its input. Training-mode BatchNorm multiplies an absolute error by
        (var + eps)^-1/2, up to 31.6 on a column that hardly moves, so a reference computed from
        the features is a tight one only where this stays near 1. -> {layer: factor}"""
        rng = np.random.default_rng(seed)
        out = {}
        for si, (kind, lines, gov, gkind) in enumerate(self.stages):
            if gov is None or si == 0:
                continue
            x = self.stage_in[si].astype(np.float64)
            xp = f16(x + delta * np.sqrt((x * x).mean()) * rng.standard_normal(x.shape)).astype(np.float32)
            y, net = self._stage_forward(si, xp, None, False)
            if net is not None:
                net.close()
            y0 = self.stage_out[si]
            out[gov] = (np.linalg.norm(y - y0) / np.linalg.norm(y0)) / (np.linalg.norm(xp - x) / np.linalg.norm(x))
        return out

    def act(self, name):
        return self.acts[name]

    def backward(self, out_grad):
        g = np.ascontiguousarray(out_grad, np.float32)
        grads = {}
        for si in range(len(self.stages) - 1, -1, -1):
            kind, lines, gov, gkind = self.stages[si]
            x, net = self.stage_in[si], self.nets[si]
            if kind == "prefinal":
                gW, gb, gW2, gin = prefinal_backward(g.astype(np.float64), self.fwd[gov])
                grads[gov + ".BigW"], grads[gov + ".BigBias"], grads[gov + ".SmallW"] = gW, gb.reshape(1, -1), gW2
                g = gin.astype(np.float32)
                continue
            gtop = g
            if gov is not None:
                f = self.fwd[gov]
                gtop = bn_block_backward(g, f["r"], f["H"], f["F"], f["scale"], f["shift"])[2].astype(np.float32)
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

    def _ivector_gradient(self, net, grads):
        """a governed per-sequence batchnorm-component: ivector-linear's weight gradient through it"""
        for name, (r, rms, src) in self.comp_in.items():
            if "ReplaceIndex" not in self.layer_line[src]:
                continue
            comb = [l for l in self.lines if l.split()[0] == "combine-feature-maps-layer" and name in l]
            assert len(comb) == 1
            kv = _kv(comb[0])
            ci = net.index[kv["name"]]
            T, w = net.net.T, net.L[ci]["out_dim"]
            gc = np.ctypeslib.as_array(net.net.gact[ci], shape=(T * w,)).reshape(T, w)
            grads[src + ".W"] = ivector_branch_backward(gc, self.seq_off, int(kv["height"]), int(kv.get("num-filters1", 1)),
                                                        int(kv.get("num-filters2", 1)), r, rms, self.ivec)

    def close(self):
        for net in self.nets:
            if net is not None:
                net.close()
        self.nets = []
