"""Reference of the TDNN-F per-sequence dropout: Kaldi's
GeneralDropoutComponent with continuous=true, time-period=0, block-dim=dim.

- philox4x32_10: the counter-based generator (Salmon, Moraes, Dror, Shaw: "Parallel random
  numbers: as easy as 1, 2, 3", SC'11) in numpy, checked against the Random123 known-answer
  vectors in test_dropout_ref.py.
- dropout_masks: the mask rule of kf_ops.h kf_dropout_masks.
- row_segments: the row -> sequence map of kf_ops.h kf_row_seg.
- DropoutOracle: forward / backward of a network whose tdnnf-layers carry masks, built from
  the committed CPU oracle (oracle/oracle.py OracleNet, imported, not edited) run one layer at
  a time, the mask inserted at the two places of the rule.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: two ints (or uint32 [..., 2]) -> uint32 [..., 4]"""
    c = np.asarray(counter, np.uint64) & _U32
    k = np.asarray(key, np.uint64) & _U32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # < 2^64: exact in uint64
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _U32, p1 & _U32, ((p0 >> 32) ^ c3 ^ k1) & _U32, p0 & _U32
        k0, k1 = (k0 + W0) & _U32, (k1 + W1) & _U32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def dropout_masks(seed: int, step: int, ordinal: int, B: int, dim: int, p: float) -> np.ndarray:
    """mask [B x dim] float32: x = Philox4x32-10(counter = {step, ordinal, b, n // 4}, key = the
    seed's low and high words)[n % 4], u = (x >> 8) 2^-24, m = 4p u + (1 - 2p) in fp32 (the
    device fuses the multiply-add: the two agree to 1 ulp)."""
    assert dim % 4 == 0
    b, j = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(dim // 4, dtype=np.uint64), indexing="ij")
    ctr = np.stack([np.full_like(b, step & _U32), np.full_like(b, ordinal), b, j], axis=-1)
    x = philox4x32_10(ctr, np.array([seed & _U32, (seed >> 32) & _U32], np.uint64))
    u = (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    p = np.float32(p)
    a, o = np.float32(4.0) * p, np.float32(1.0) - np.float32(2.0) * p
    return (a * u + o).astype(np.float32).reshape(B, dim)


def row_segments(seq_row0, T: int, tc0: int = 0, tc: int = 0) -> np.ndarray:
    """The sequence of every GEMM row: the T frames, or with tc > 0 the compact rows of the
    row-subsampled step (row c is frame 3c for c < tc0, else (T-1) - 3(tc-1-c))."""
    so = np.asarray(seq_row0, np.int64)
    rows = np.arange(T) if tc <= 0 else np.array([3 * c if c < tc0 else (T - 1) - 3 * (tc - 1 - c) for c in range(tc)])
    return (np.searchsorted(so, rows, side="right") - 1).astype(np.int32)


def epilogue_drop_ref(acc, mag, K, drop, row_seg, scale=None, shift=None, scale2=None, **kw):
    """gemm_ref.epilogue_ref extended with KfEpilogue.drop (kf_ops.h): D[m][n] = drop[row_seg[m]][n]
    multiplies the BatchNorm output when the launch has scale (the forward), else out2's value
    (the input gradient). (relu scale + shift) D = relu (scale D) + shift D, and v scale2 D =
    v (scale2 D), so the rule is gemm_ref's with row-expanded parameters; its bound then carries
    |D| as it carries |scale| and |scale2|. The kernel's extra fp32 multiply rounds once more:
    2^-24 relative on the product, and 2^-24 on the BatchNorm intermediate relu scale + shift it
    multiplies, which the reference's bound (that treats the shift as exact) does not hold; both
    are added here, on the magnitudes they apply to."""
    import gemm_ref
    f = np.float64
    D = np.asarray(drop, f)[np.asarray(row_seg)]
    if scale is not None:
        r = gemm_ref.epilogue_ref(acc, mag, K, scale=scale.astype(f)[None, :] * D, shift=shift.astype(f)[None, :] * D,
                                  scale2=scale2, **kw)
        pre = np.maximum(r["pre"], 0.0) if r["bits"] is not None else r["pre"]
        extra = 2.0 ** -23 * (np.abs(pre * scale.astype(f)) + np.abs(shift.astype(f))) * np.abs(D)
        r["bound"] = r["bound"] + extra
        r["tol"] = r["tol"] + extra
        return r
    s2 = D if scale2 is None else scale2.astype(f)[None, :] * D
    r = gemm_ref.epilogue_ref(acc, mag, K, scale2=s2, **kw)
    extra = 2.0 ** -23 * np.abs(r["out2"])
    r["bound2"] = r["bound2"] + extra
    r["tol2"] = r["tol2"] + extra
    return r


class DropoutOracle:
    """The oracle's network with a dropout mask on tdnnf-layers, one OracleNet per stage.

    A tdnnf-layer with a mask is run once per sequence b on ALL rows (its splice reads across
    sequence boundaries, as the product's does) with its BatchNorm's gamma and beta multiplied by
    m[b]: (relu(z) scale + shift) m = relu(z) (scale m) + shift m, so the oracle's own fused
    epilogue applies the mask after the BatchNorm and before the bypass, and its backward
    forms dz = g (scale m) relu_bit. Rows of sequence b are taken from run b; in the backward run
    b sees the output gradient of sequence b's rows only and the runs' gradients are summed.
    A stage begins with an identity linear-component (exact on fp16 values), whose stored
    output gradient is the stage's input gradient.

    Its own error against the rule: scale m and shift m are rounded to fp32 before the fused
    multiply-add (a few fp32 ulps), and a stage hands down the fp16-rounded input gradient
    where the product's epilogue forms dz from the unrounded sum (one fp16 rounding, 2^-11
    relative, per layer): both far below the 2e-3 / 5e-3 bounds the comparisons use.
    """

    def __init__(self, xconfig: str, params: dict, bns: dict, masks: dict, seq_row0, threads=8):
        import oracle
        self.oracle = oracle
        self.params, self.bns, self.masks = params, bns, masks
        self.seq = np.asarray(seq_row0, np.int64)
        self.threads = threads
        inputs, lines = [], []
        for raw in xconfig.splitlines():
            line = raw.strip()
            if not line or line.startswith("#"):
                continue
            (inputs if line.split()[0] == "input" else lines).append(line)
        assert len(inputs) == 1, "one input"
        # stages: runs of layers without a mask, and each masked tdnnf-layer on its own
        self.stages, cur = [], []
        for line in lines:
            name = dict(t.split("=", 1) for t in line.split()[1:] if "=" in t)["name"]
            if name in masks:
                if cur:
                    self.stages.append((cur, None))
                self.stages.append(([line], name))
                cur = []
            else:
                cur.append(line)
        if cur:
            self.stages.append((cur, None))
        self.first_input = inputs[0]
        self.acts, self.stage_in, self.nets = {}, [], []

    def _net(self, si, din, bn_over=None):
        lines, _ = self.stages[si]
        params, bns = dict(self.params), dict(self.bns)
        if si == 0:
            text = "\n".join([self.first_input] + lines) + "\n"
        else:
            text = "\n".join([f"input name=input dim={din}", f"linear-component name=stage-in dim={din}"] + lines) + "\n"
            params["stage-in.W"] = np.eye(din, dtype=np.float32)
        if bn_over:
            bns.update(bn_over)
        return self.oracle.OracleNet(text, params, bns, round_mode=self.oracle.ROUND_FUSED, threads=self.threads)

    def _bn_masked(self, name, m):
        mean, var, gamma, beta = self.bns[(name, 0)]
        return {(name, 0): (mean, var, (gamma * m).astype(np.float32), (beta * m).astype(np.float32))}

    def forward(self, features, force_masks=None):
        x = np.ascontiguousarray(features, np.float32)
        T = x.shape[0]
        self.stage_in, self.nets = [], []
        for si, (lines, masked) in enumerate(self.stages):
            self.stage_in.append(x)
            names = [dict(t.split("=", 1) for t in l.split()[1:] if "=" in t)["name"] for l in lines]
            fm = {n: force_masks[n] for n in names if force_masks and n in force_masks} or None
            if masked is None:
                net = self._net(si, x.shape[1])
                net.forward(x, force_masks=fm)
                for n in names:
                    self.acts[n] = net.act(n)
                self.nets.append([net])
                x = net.act(names[-1])
                continue
            m = self.masks[masked]
            y, runs = None, []
            for b in range(len(self.seq) - 1):
                net = self._net(si, x.shape[1], self._bn_masked(masked, m[b]))
                net.forward(x, force_masks=fm)
                a = net.act(masked)
                y = np.zeros_like(a) if y is None else y
                r0, r1 = int(self.seq[b]), int(self.seq[b + 1])
                y[r0:r1] = a[r0:r1]
                runs.append(net)
            assert int(self.seq[-1]) == T
            self.acts[masked] = y
            self.nets.append(runs)
            x = y
        return x

    def act(self, name):
        return self.acts[name]

    def backward(self, out_grad):
        """-> gradients keyed by the product's parameter names"""
        g = np.ascontiguousarray(out_grad, np.float32)
        grads = {}
        for si in range(len(self.stages) - 1, -1, -1):
            lines, masked = self.stages[si]
            x = self.stage_in[si]
            gin = None
            for b, net in enumerate(self.nets[si]):
                gb = g
                if masked is not None:
                    gb = np.zeros_like(g)
                    r0, r1 = int(self.seq[b]), int(self.seq[b + 1])
                    gb[r0:r1] = g[r0:r1]
                net.backward(gb)
                for k, v in net.grads().items():
                    if not k.startswith("stage-in."):
                        grads[k] = grads.get(k, 0) + v
                if si > 0:
                    d = x.shape[1]
                    gi = np.ctypeslib.as_array(net.net.gact[0], shape=(x.shape[0] * d,)).reshape(-1, d).copy()
                    gin = gi if gin is None else gin + gi
            g = gin
        return grads

    def close(self):
        for runs in self.nets:
            for net in runs:
                net.close()
        self.nets = []
