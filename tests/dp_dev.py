"""Shared helpers of tests/test_gpu_dp_modes.py: the two one-GPU proofs of the data-parallel bucket
gates (tests/test_gpu_dp.py states them on two networks at full rows) on a net in any mode of the
train step, with tests/history_dev.py's networks and switches.

SNAPSHOT proof: the gradient buffer is filled with 0xFF bytes and the snapshot with 0x7F, the bound
backward runs, and every bucket's snapshot (taken on the communication stream as its exchange
starts) equals the finished gradient bit for bit. PEER_MEAN proof: every exchanged bucket is averaged
with a second shard's gradient; the bound step followed at once by nnet_sgd gives (gA + gB) * 0.5 and
the weights of one SGD step on that mean, bit for bit. Each has the negative control of
nnet_dp_debug_early: every bucket exchanged before the backward must show.

Every comparison is bit for bit, against the unbound backward of the same net in the same mode or
against the float32 mean computed on the host."""
import numpy as np

import history_dev as hd

BUCKET = 16 << 10      # bytes: at most one tensor group per bucket on these nets
LR, MOM = 1e-3, 0.9
SEEDS_A, SEEDS_B = (1234, 7), (4321, 8)     # (features, output gradient) of the two shards
MID_BN = ("prefinal-layer name=prefinal-chain input=prefinal-l",
          "batchnorm-component name=mid-bn input=prefinal-l\nprefinal-layer name=prefinal-chain input=mid-bn")


def midbn_xcfg():
    """configs/tiny.xconfig with a batchnorm-component between prefinal-l and prefinal-chain: the
    pass-through step of the backward (backward.cpp, step(), case LayerType::Batchnorm), with
    trainable layers above (prefinal-chain, output) and below it (prefinal-l, tdnnf8 ...)"""
    from kfp16 import synth
    x = synth.load_xconfig("tiny.xconfig")
    assert MID_BN[0] in x
    return x.replace(*MID_BN)


def xconfig(name):
    return midbn_xcfg() if name == "midbn" else hd.xconfig(name)


class Case:
    """a network (by name), T, the switches of its mode, and what the net must report so that the
    case reaches the code it is for. nt: the tail depth of the row set (None: full rows);
    conv, conv_rows: the conv below the row set and the rows it holds ("compact" / "full"); seq: the sequence
    boundaries of nnet_forward_ivector; offpath: tensors a chain-only backward zero-fills."""

    def __init__(self, name, cfg, T, *switches, nt=None, tail=None, conv=None, conv_rows=None, seq=None,
                 offpath=(), two_stream=True):
        self.name, self.cfg, self.T, self.switches = name, cfg, T, switches
        self.nt, self.tail, self.conv, self.conv_rows = nt, tail, conv, conv_rows
        self.seq, self.offpath = seq, tuple(offpath)
        self.two_stream = two_stream

    def one_stream(self):
        return Case(self.name + "-one-stream", self.cfg, self.T, *self.switches, nt=self.nt, tail=self.tail,
                    conv=self.conv, conv_rows=self.conv_rows, seq=self.seq, offpath=self.offpath, two_stream=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Shard:
    """one rank's minibatch: features (and ivectors), and the output gradient on the rows
    0 (mod 3), uploaded in the forward's row form at the first forward"""

    def __init__(self, kf, case, seeds, P=200):
        self.feats = kf.upload_fp16(hd.features(case.T, seeds[0]))
        self.iv = None
        if case.seq is not None:
            B = len(case.seq) - 1
            self.iv = kf.upload_fp16((np.random.default_rng(seeds[0] + 31 * B).standard_normal((B, 100)) * 2)
                                     .astype(np.float16))
        self.og_host = hd.out_grad(case.T, seed=seeds[1], P=P)
        self.og = None


class Rig:
    """a live net of a case"""

    def __init__(self, kf, case):
        from kfp16 import synth
        self.kf, self.case = kf, case
        self.net = kf.Network(xconfig(case.cfg), max_frames=hd.MAXF)
        synth.init_network(self.net)
        self.net.set_wgrad_stream(case.two_stream)
        for s in case.switches:
            s.on(self.net)
        self.P = self.net.num_params
        self.A, self.B = Shard(kf, case, SEEDS_A), Shard(kf, case, SEEDS_B)
        self.w0 = self.net.get_params()

    def close(self):
        self.net.close()

    def forward(self, sh, scale=None):
        """the generators pinned, the forward, and the shard's output gradient in its row form
        (times `scale`, as an objective under the loss scale would hand it over)"""
        net, c = self.net, self.case
        net.set_dropout_step(3)
        net.set_spec_augment_step(3)
        if c.seq is not None:
            net.forward_ivector(sh.feats.ptr, c.T, sh.iv.ptr, np.asarray(c.seq, np.int32))
        else:
            net.forward(sh.feats.ptr, c.T)
        tc, tc0, rows = net.row_set()
        og = sh.og_host[rows] if tc else sh.og_host
        if scale is not None:
            scaled = og.astype(np.float32) * np.float32(scale)
            assert np.abs(scaled).max() < 65504
            return self.kf.upload_fp16(scaled.astype(np.float16))
        if sh.og is None:
            sh.og = self.kf.upload_fp16(og)
        return sh.og

    def fill(self, ptr, byte):
        self.kf.core.bridge_gpu_memset(ptr, byte, self.P * 4)

    def read(self, ptr):
        return self.kf.read_f32(ptr, (self.P,)).copy()

    def grad(self, sh, scale=None):
        """the gradient buffer (zero first) after forward and backward of a shard"""
        og = self.forward(sh, scale)
        self.fill(self.net.grad_ptr, 0)
        self.net.backward(og.ptr)
        self.kf.sync()
        return self.read(self.net.grad_ptr)

    def ranges(self, names=None):
        return {k: (off, off + r * c) for k, (r, c, off) in self.net.params.items() if names is None or k in names}

    def reach(self):
        """after a forward: the case runs the rows (and so the launches) it names"""
        net, c = self.net, self.case
        tc, tc0, _ = net.row_set()
        if c.nt is None:
            assert (tc, tc0) == (0, 0)
            return
        want = hd.expected_row_set(c.T, c.nt)
        assert (tc, tc0) == want and tc0 > 0, (c.name, (tc, tc0), want)
        assert (tc > tc0) == c.tail, (c.name, tc, tc0)
        rows = net.activation(c.conv)[1]
        assert rows == (tc if c.conv_rows == "compact" else c.T), (c.name, rows, tc)

    def plan(self, min_buckets=4):
        from kfp16 import dp
        plan = self.net.dp_plan(BUCKET)
        assert dp.covers_exactly(plan, self.P), self.case.name
        assert len(plan) >= min_buckets, (self.case.name, len(plan))
        return plan


class Bound:
    """the net bound to the communicator with a debug hook on, and everything undone on the way out"""

    def __init__(self, rig, comm, mode, aux_ptr):
        self.rig, self.comm, self.mode, self.aux = rig, comm, mode, aux_ptr

    def __enter__(self):
        net = self.rig.net
        net.bind_dp(self.comm, BUCKET)
        self.comm.debug(self.mode, net.grad_ptr, self.aux, self.rig.P)
        return self

    def __exit__(self, *exc):
        net = self.rig.net
        self.rig.kf.sync()
        net.dp_debug_early(False)
        self.comm.debug(0)
        net.bind_dp(None, 0)
        return False


def repeatable(rig):
    """two unbound runs of shard A give the same gradient bits -> that gradient"""
    ga, again = rig.grad(rig.A), rig.grad(rig.A)
    rig.reach()
    differ = [k for k, (b, e) in rig.ranges().items() if not np.array_equal(bits(ga[b:e]), bits(again[b:e]))]
    assert not differ, "%s: the unbound backward does not repeat its bits in %s" % (rig.case.name, differ)
    np.testing.assert_array_equal(bits(ga), bits(again))
    return ga


def snapshot_proof(rig, comm, plan, ga):
    """every bucket's exchange starts from its finished gradient; the early control does not"""
    kf, net, P = rig.kf, rig.net, rig.P
    snap = kf.DeviceBuffer(P * 4)
    launches0 = comm.stats()[0]

    def run(early):
        net.dp_debug_early(early)
        og = rig.forward(rig.A)
        rig.fill(net.grad_ptr, 0xFF)        # NaN everywhere: unwritten values show
        rig.fill(snap.ptr, 0x7F)
        net.backward(og.ptr)
        kf.sync()
        g, s = bits(rig.read(net.grad_ptr)), bits(rig.read(snap.ptr))
        return g, s, [j for j, (_, b, e) in enumerate(plan) if not np.array_equal(g[b:e], s[b:e])]

    with Bound(rig, comm, comm.DEBUG_SNAPSHOT, snap.ptr):
        g, s, bad = run(False)
        assert comm.stats()[0] - launches0 == len(plan)
        assert not bad, "%s: buckets exchanged before their gradients were final: %s of %d" % (rig.case.name, bad[:10], len(plan))
        # the gradient itself was produced (no NaN left outside the 64-element pads), and it is
        # the unbound backward's
        for name, (b, e) in rig.ranges().items():
            assert np.isfinite(g[b:e].view(np.float32)).all(), name
            np.testing.assert_array_equal(g[b:e], bits(ga[b:e]), err_msg=name)
        # off-path tensors: zero-filled before their bucket left, not the 0xFF prefill
        for name, (b, e) in rig.ranges(rig.case.offpath).items():
            assert not s[b:e].any() and not g[b:e].any(), name
        _, _, bad_early = run(True)
        assert bad_early, "negative control: issuing every bucket before the backward went unnoticed"
    snap.free()


def peer_mean_proof(rig, comm, ga):
    """the bound step on shard A with shard B's gradient as the peer's, then SGD with no sync in
    between: the gradient (gA + gB) * 0.5 and the weights of an SGD step on it"""
    kf, net, P = rig.kf, rig.net, rig.P
    gb = rig.grad(rig.B)
    assert not np.array_equal(ga, gb)
    off = rig.ranges(rig.case.offpath)
    rng = np.random.default_rng(5)
    for name, (b, e) in off.items():
        # (a chain-only backward leaves zeros there on every rank; a peer value that is not zero
        # shows whether the range was exchanged at all)
        assert not ga[b:e].any() and not gb[b:e].any(), name
        gb[b:e] = rng.standard_normal(e - b).astype(np.float32)
    mean = ((ga + gb) * np.float32(0.5)).astype(np.float32)

    # reference: one SGD step on the mean gradient (no exchange)
    net.set_params(rig.w0)
    kf.check(kf.core.bridge_transfer_float32(net.grad_ptr, mean.ctypes.data, P), "upload mean")
    net.sgd(LR, MOM)
    kf.sync()
    w_ref = rig.read(net.master_ptr)
    peer = kf.upload_f32(gb)

    def bound_step(early):
        net.set_params(rig.w0)
        net.dp_debug_early(early)
        og = rig.forward(rig.A)
        rig.fill(net.grad_ptr, 0)
        net.backward(og.ptr)
        net.sgd(LR, MOM)            # enqueued behind kf_dp_join, no host sync between
        kf.sync()
        return rig.read(net.grad_ptr), rig.read(net.master_ptr)

    with Bound(rig, comm, comm.DEBUG_PEER_MEAN, peer.ptr):
        g, w = bound_step(False)
        np.testing.assert_array_equal(bits(g), bits(mean))
        np.testing.assert_array_equal(bits(w), bits(w_ref))
        for name, (b, e) in off.items():
            np.testing.assert_array_equal(g[b:e], gb[b:e] * np.float32(0.5), err_msg=name)
        g_early, _ = bound_step(True)
        assert not np.array_equal(bits(g_early), bits(mean)), "negative control: early exchange went unnoticed"
    net.set_params(rig.w0)
    peer.free()
