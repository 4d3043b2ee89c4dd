"""Shared helpers of tests/test_gpu_history.py (and the tiny3 xconfig test_gpu_bn_rows.py uses): the
networks, the switches, one forward / backward step with everything it leaves read back, and the
bit-for-bit comparison with a fresh net.

A fresh net (Recipe.make, fresh): a new Network of the same xconfig, max_frames, init_network seed
and switches that runs the compared step as its first step. Its snapshots are computed once per
(recipe, capacity, step) and shared by the tests; nobody writes to them."""
import contextlib
import os

import numpy as np

MAXF = 300
SEED = 0x5EED5EED12345678
STRIDE1 = "name=tdnnf8 dim=256 bottleneck-dim=64 time-stride=1"
CNN4 = ("conv-relu-batchnorm-layer name=cnn4 height-in=20 height-out=10 height-subsample-out=2 time-offsets=-1,0,1 "
        "height-offsets=-1,0,1 num-filters-out=64")
CNN5 = ("conv-relu-batchnorm-layer name=cnn5 height-in=10 height-out=10 time-offsets=-1,0,1 height-offsets=-1,0,1 "
        "num-filters-out=128")
DISTURB_SEED, DISTURB_AMP = 99, 4.0


# ---------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------
def tiny3_xcfg(dropout=False, base="tiny.xconfig"):
    """configs/tiny.xconfig (or another config with its TDNN-F stack) with tdnnf8 at time-stride 3:
    tdnnf5 .. output then form the row set of nnet_set_row_subsampling above cnn4, with three
    3-strided layers (a tail of 3 + 4 = 7 rows). dropout: a dropout component (proportion 0) on
    every TDNN-F layer with a bypass."""
    from kfp16 import synth
    x = synth.load_xconfig(base)
    assert STRIDE1 in x
    x = x.replace(STRIDE1, STRIDE1.replace("time-stride=1", "time-stride=3"))
    assert x.count("bypass-scale=0.66") == 4
    return x.replace("bypass-scale=0.66", "bypass-scale=0.66 dropout-proportion=0.0") if dropout else x


def tiny3c_xcfg():
    """tiny3 with a cnn5 at height 10 -> 10 and 128 filters above cnn4 (the benchmark model's cnn6 at
    half its filters): the conv below the row set then runs on the compact rows itself
    (KfNet.conv_c), which tiny3's cnn4, subsampling the height, never does"""
    x = tiny3_xcfg()
    assert CNN4 in x
    return x.replace(CNN4, CNN4 + "\n" + CNN5)


def tiny3w_xcfg():
    """tiny3 with cnn4 at height 20 -> 20 and 64 filters: no height subsampling, but the time-strided
    halo of its weight gradient over the compact rows is too large for the halo kernel, so
    nnet_set_row_subsampling leaves it on full rows"""
    x = tiny3_xcfg()
    assert CNN4 in x
    return x.replace(CNN4, CNN4.replace("height-out=10 height-subsample-out=2", "height-out=20"))


def top_conv(cfg):
    """the conv layer below the TDNN-F stack"""
    return "cnn5" if cfg == "tiny3c" else "cnn4"


def xent3_xcfg():
    """configs/tiny_xent.xconfig (tdnnf4 at stride 3 above cnn2: one 3-strided layer, a tail of 5
    rows) with a dropout component on its TDNN-F layers"""
    from kfp16 import synth
    x = synth.load_xconfig("tiny_xent.xconfig")
    assert x.count("bypass-scale=0.66") == 2
    return x.replace("bypass-scale=0.66", "bypass-scale=0.66 dropout-proportion=0.0")


def sa2_xcfg():
    """tiny with a spec-augment layer between tdnnf8 and prefinal-l, whose consumer would read an
    MXFP8 copy (test_gpu_specaug_net.py's conflict case)"""
    from kfp16 import synth
    old = "linear-component name=prefinal-l dim=64"
    x = synth.load_xconfig("tiny.xconfig")
    assert old in x
    return x.replace(old, "spec-augment-layer name=sa2\n" + old)


def xconfig(name):
    from kfp16 import synth
    made = {"tiny3": tiny3_xcfg, "tiny3d": lambda: tiny3_xcfg(True), "tiny3c": tiny3c_xcfg, "tiny3w": tiny3w_xcfg, "xent3d": xent3_xcfg,
            "sa2": sa2_xcfg, "specaug": lambda: synth.load_xconfig("specaug/tiny_specaug.xconfig"),
            "specaug3": lambda: tiny3_xcfg(base="specaug/tiny_specaug.xconfig")}
    return made[name]() if name in made else synth.load_xconfig(name + ".xconfig")


def features(T, seed=1234, amp=1.0):
    from kfp16 import synth
    return (synth.make_features(T, 40, seed=seed).astype(np.float32) * amp).astype(np.float16)


def out_grad(T, seed=7, P=200):
    """on the rows 0 (mod 3) only: what row subsampling declares"""
    og = np.zeros((T, P), np.float16)
    og[::3] = (np.random.default_rng(seed).standard_normal((len(og[::3]), P)) * 0.05).astype(np.float16)
    return og


def expected_row_set(T, nt, on=True, max_frames=MAXF):
    """(tc, tc0) by forward_impl's rule (forward.cpp): the rows 0 (mod 3), and a tail of nt rows
    unless (T - 1) % 3 == 0; full rows (0, 0) below tc0 = 4 * tail + 16 or above the capacity"""
    if not on:
        return 0, 0
    tail = 0 if (T - 1) % 3 == 0 else nt
    tc0 = (T - 1) // 3 + 1
    cap = (max_frames - 1) // 3 + 1 + nt
    return (tc0 + tail, tc0) if tc0 >= 4 * tail + 16 and tc0 + tail <= cap else (0, 0)


# ---------------------------------------------------------------------------
# switches
# ---------------------------------------------------------------------------
@contextlib.contextmanager
def rsub_conv_env(value):
    """KF_RSUB_CONV around nnet_set_row_subsampling, as test_gpu_row_subsampling._run sets it"""
    if value is not None:
        os.environ["KF_RSUB_CONV"] = value
    try:
        yield
    finally:
        os.environ.pop("KF_RSUB_CONV", None)


class Switch:
    """a mode of the train step: how it is switched on and off; kind names what a step under it
    leaves besides activations and gradients ("drop", "sa", "bn")"""

    def __init__(self, name, on, off, kind=None):
        self.name, self.on, self.off, self.kind = name, on, off, kind


def fp8(mode):
    return Switch("fp8-%d" % mode, lambda n: n.set_fp8(True if mode == 1 else mode), lambda n: n.set_fp8(False))


IMPLICIT = Switch("implicit-dz", lambda n: n.set_implicit_dz(True), lambda n: n.set_implicit_dz(False))
WGRAD = Switch("one-stream", lambda n: n.set_wgrad_stream(False), lambda n: n.set_wgrad_stream(True))
NATGRAD = Switch("natgrad", lambda n: n.set_natural_gradient(True), lambda n: n.set_natural_gradient(False))
SPECAUG = Switch("specaug", lambda n: n.set_spec_augment(True, SEED), lambda n: n.set_spec_augment(False), "sa")


def rsub(conv=None):
    def on(n):
        with rsub_conv_env(conv):
            n.set_row_subsampling(3)
    return Switch("rsub" if conv is None else "rsub-conv" + conv, on, lambda n: n.set_row_subsampling(0))


def _drop_on(n):
    n.set_dropout_proportion(0.3)
    n.set_dropout(True, SEED)


DROPOUT = Switch("dropout", _drop_on, lambda n: n.set_dropout(False), "drop")


def bn_train(sites="tdnnf", rows="all"):
    def on(n):
        n.set_batchnorm_train_rows(rows)
        n.set_batchnorm_train_sites(sites)
        n.set_batchnorm_train(True)
    return Switch("bn-%s-%s" % (sites, rows), on, lambda n: n.set_batchnorm_train(False), "bn")


# ---------------------------------------------------------------------------
# a live net
# ---------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def same(a, b, what=""):
    """two snapshots, bit for bit (np.array_equal on the unsigned views)"""
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    bad = [k for k in a if a[k].shape != b[k].shape or not np.array_equal(_bits(a[k]), _bits(b[k]))]
    assert not bad, "%s: %d of %d tensors differ: %s" % (what, len(bad), len(a), bad[:10])


def differ(a, b):
    return [k for k in a if k in b and (a[k].shape != b[k].shape or not np.array_equal(_bits(a[k]), _bits(b[k])))]


class Live:
    def __init__(self, kf, xcfg, max_frames=MAXF):
        from kfp16 import synth
        self.kf, self.xcfg = kf, xcfg
        self.net = kf.Network(xcfg, max_frames=max_frames)
        self.params, self.bns = synth.init_network(self.net)
        self.on = {}
        names = [l[0] for l in self.net.layers]
        self.names = names
        convs = [n for n, ty, *_ in self.net.layers if ty == 6]
        tdnnf = [n for n, ty, *_ in self.net.layers if ty == 7]
        # one conv layer (the top of the conv stack) and one TDNN-F layer above it
        self.inner = [convs[-1], tdnnf[min(1, len(tdnnf) - 1)]]
        self.ivec = "ivector-linear" in names
        self.xent = "output-xent" in names

    def switch(self, sw, on=True):
        (sw.on if on else sw.off)(self.net)
        if on:
            self.on[sw.name] = sw
        else:
            self.on.pop(sw.name, None)
        return self

    def kinds(self):
        return {s.kind for s in self.on.values() if s.kind}

    def governed(self):
        out = []
        for n in self.net.batchnorm_train_layers():
            out.append((n, 0))
            if n.startswith("prefinal"):
                out.append((n, 1))
        return out

    def bn_counts(self):
        return {k: self.net.batchnorm_stats(*k)[0] for k in self.governed()}

    def bn_rows(self, key, T):
        """the rows (block rows of a conv) one forward adds to a governed BatchNorm's count: the rows
        c < tc0 of a compact layer in a compact forward, else every row the layer holds"""
        net = self.net
        tc, tc0, _ = net.row_set()
        rows = net.activation(key[0])[1]
        dims = {n: dout for n, _ty, _din, dout in net.layers}
        h = dims[key[0]] // net._bn_dim(*key) if key[0] in [n for n, ty, *_ in net.layers if ty == 6] else 1
        per_seq = {"ivector-linear", "ivector-batchnorm"}
        assert key[0] not in per_seq
        return (tc0 if tc and rows == tc else T) * h

    def step(self, T, seq=None, feat_seed=1234, amp=1.0, pin=3, two_seeds=False, want_rows=None, backward=True):
        """one forward / backward at T frames -> the snapshot. seq: the sequence boundaries
        (nnet_set_sequences, or nnet_forward_ivector's); the generators are pinned to step `pin`
        immediately before the forward; the output gradient (out_grad: rows 0 (mod 3)) goes in the
        forward's row form; two_seeds: nnet_backward_xent with a second such seed."""
        kf, net = self.kf, self.net
        fb = kf.upload_fp16(features(T, feat_seed, amp))
        if seq is not None and not self.ivec:
            net.set_sequences(np.asarray(seq, np.int32))
        net.set_dropout_step(pin)
        net.set_spec_augment_step(pin)
        B = 0
        if self.ivec:
            B = len(seq) - 1
            iv = (np.random.default_rng(feat_seed + 31 * B).standard_normal((B, 100)) * 2 * amp).astype(np.float16)
            ib = kf.upload_fp16(iv)
            net.forward_ivector(fb.ptr, T, ib.ptr, np.asarray(seq, np.int32))
        else:
            net.forward(fb.ptr, T)
        tc, tc0, rows = net.row_set()
        if want_rows is not None:
            assert (tc, tc0) == tuple(want_rows), (T, (tc, tc0), want_rows)
        snap = {"rows": np.asarray([tc, tc0], np.int32)}
        acts = ["output"] + self.inner + (["output-xent"] if self.xent else [])
        for n in acts:
            snap["act/" + n] = net.read_activation(n)
        for n in ("ivector-linear", "ivector-batchnorm") if self.ivec else ():
            snap["act/" + n] = net.read_activation(n)[:B]
        for n, m in net.relu_masks().items():
            # (relu_masks reads T rows of every layer: a layer on the compact rows holds fewer)
            w = m.size // T
            snap["relu/" + n] = m[:net.activation(n)[1] * w]
        kinds = self.kinds()
        if "drop" in kinds:
            for n in net.dropout_layers():
                snap["drop/" + n] = net.dropout_mask(n)
        if "sa" in kinds:
            for n in net.spec_augment_layers():
                snap["sa/" + n] = net.spec_augment_rows(n)
        if "bn" in kinds:
            for k in self.governed():
                m, v = net.batchnorm_batch_stats(*k)
                snap["bn-mean/%s/%d" % k], snap["bn-var/%s/%d" % k] = m, v
        if not backward:
            return snap
        og = out_grad(T)
        gb = kf.upload_fp16(og[rows] if tc else og)
        if two_seeds:
            xg = out_grad(T, seed=8)
            xb = kf.upload_fp16(xg[rows] if tc else xg)
            net.backward(gb.ptr, xb.ptr)
        else:
            net.backward(gb.ptr)
        for k, g in net.read_grads().items():
            snap["grad/" + k] = g
        if self.ivec:
            li = self.names.index("combine_inputs")
            snap["gdb"] = kf.read_fp16(kf.nnet.nnet_debug_tensor(net.h, b"gdb", li), (B, 200))
        return snap

    def disturb(self, T, seq=None, two_seeds=False):
        """the step before a compared one: other features at four times the amplitude (and another
        T), so that what it leaves beyond the next T, or in shared ring slots, is unrelated data"""
        return self.step(T, seq=seq, feat_seed=DISTURB_SEED, amp=DISTURB_AMP, pin=11, two_seeds=two_seeds)

    def close(self):
        self.net.close()


class Recipe:
    """an xconfig (by name, xconfig()) and the switches a net of it has on"""

    def __init__(self, cfg, *switches):
        self.cfg, self.switches = cfg, switches
        self.key = (cfg,) + tuple(s.name for s in switches)

    def make(self, kf, max_frames=MAXF):
        live = Live(kf, xconfig(self.cfg), max_frames)
        for s in self.switches:
            live.switch(s)
        return live

    def plus(self, *more):
        return Recipe(self.cfg, *(self.switches + more))


_fresh = {}


def fresh(kf, recipe, T, max_frames=MAXF, **kw):
    """the snapshot of step(T, **kw) as the first step of a fresh net of the recipe (shared: read only)"""
    key = (recipe.key, max_frames, T, tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple, np.ndarray)) else v)
                                                   for k, v in kw.items() if k != "want_rows")))
    if key not in _fresh:
        live = recipe.make(kf, max_frames)
        try:
            _fresh[key] = live.step(T, **kw)
        finally:
            live.close()
        for v in _fresh[key].values():
            v.setflags(write=False)
    return _fresh[key]
