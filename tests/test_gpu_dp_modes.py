"""The data-parallel bucket gates of nnet_backward (tests/test_gpu_dp.py) on the row-subsampled step
and under the other modes of the train step, on one MI355X: row subsampling in its four conv forms,
the one-stream backward, implicit dz, the batchnorm-component pass-through step, the
CombineFeatureMaps group with the ivector branch, attention, off-path parameters, dropout,
SpecAugment, and the loss scale. Each of them writes the gradient buffer in other launches, in
another order or on another stream than the full-row two-stream step, and at one rank a bucket
exchanged before its last writer leaves the right gradient behind: the kf_dp_debug hooks make the
order visible (tests/dp_dev.py states the two proofs and their negative controls).

Networks are small (max_frames 300, tests/history_dev.py); buckets are 16 KiB, so every group of
tensors the backward visits is a bucket of its own (7 to 12 exchanges inside one backward).
The communicator is made once for the module: creating it takes longer than any case."""
import numpy as np
import pytest

import dp_dev as dd
import history_dev as hd
from dp_dev import Case

pytestmark = pytest.mark.gpu

NT3, NT_XENT = 7, 5            # tail depth: the 3-strided layers of the row set + 4
XENT_OFFPATH = ("prefinal-xent.BigW", "prefinal-xent.BigBias", "prefinal-xent.SmallW", "output-xent.W",
                "output-xent.Bias")
RSUB = hd.rsub()

_CASES = [
    # conv_wgrad_compact's two launches (main rows, then the tail rows added), conv_window on the side stream
    Case("rsub-tail-convc", "tiny3c", 299, RSUB, nt=NT3, tail=True, conv="cnn5", conv_rows="compact"),
    # ... its single-launch form
    Case("rsub-notail-convc", "tiny3c", 298, RSUB, nt=NT3, tail=False, conv="cnn5", conv_rows="compact"),
    # the conv on full rows, read gathered; to_full_scatter
    Case("rsub-gathered", "tiny3", 299, RSUB, nt=NT3, tail=True, conv="cnn4", conv_rows="full"),
    # the halo weight gradient declined: the conv left on full rows
    Case("rsub-fullconv", "tiny3w", 299, RSUB, nt=NT3, tail=True, conv="cnn4", conv_rows="full"),
    # the compact conv switched off by KF_RSUB_CONV=0
    Case("rsub-env0", "tiny3c", 299, hd.rsub("0"), nt=NT3, tail=True, conv="cnn5", conv_rows="full"),
    Case("implicit", "tiny", 150, hd.IMPLICIT),
    # mid-bn (dp_dev.midbn_xcfg) lies between prefinal-chain and prefinal-l: both trainable
    Case("bn-pass-through", "midbn", 150),
    Case("ivector", "tiny_ivec", 150, seq=(0, 75, 150)),
    Case("attention", "tiny_att", 150),
    Case("offpath", "xent3d", 150, offpath=XENT_OFFPATH),
    Case("offpath-rsub", "xent3d", 299, RSUB, nt=NT_XENT, tail=True, conv="cnn2", conv_rows="full", offpath=XENT_OFFPATH),
    Case("dropout", "tiny3d", 299, RSUB, hd.DROPOUT, nt=NT3, tail=True, conv="cnn4", conv_rows="full"),
    Case("specaug", "specaug3", 299, RSUB, hd.SPECAUG, nt=NT3, tail=True, conv="cnn4", conv_rows="full"),
]
# the one-stream backward (nnet_set_wgrad_stream(0)): the gates are recorded on the caller's stream
_ONE_STREAM = ("rsub-tail-convc", "rsub-gathered", "ivector", "offpath")
CASES = _CASES + [c.one_stream() for c in _CASES if c.name in _ONE_STREAM]


@pytest.fixture(scope="module")
def comm(gpu):
    from kfp16 import dp
    c = dp.Communicator(0, 1, dp.unique_id(), 0)
    yield c
    c.close()


def _extra_reach(rig):
    """what a case must reach besides its row set (dp_dev.Rig.reach)"""
    net, c = rig.net, rig.case
    names = [l[0] for l in net.layers]
    if c.cfg == "tiny_ivec":
        # a bucket per group (4-byte buckets): the ivector branch's tensor lies inside one bucket,
        # alone, and that bucket is not issued before the CombineFeatureMaps step
        branch = ("ivector-linear", "ivector-batchnorm")
        walk = [n for n in reversed(names) if n not in branch]       # the chain path, top down
        (b, e), = rig.ranges(("ivector-linear.W",)).values()
        inside = [(a, lo, hi) for a, lo, hi in net.dp_plan(4) if lo <= b and e <= hi]
        assert len(inside) == 1 and inside[0][0] >= walk.index("combine_inputs"), (inside, walk)
        others = [k for k, (lo, hi) in rig.ranges().items() if k != "ivector-linear.W" and lo < inside[0][2] and inside[0][1] < hi]
        assert not others, others
    if c.cfg == "midbn":
        i = names.index("mid-bn")
        assert names[i - 1] == "prefinal-l" and names[i + 1] == "prefinal-chain"
    if c.cfg == "tiny_att":
        assert any(ty == 8 or "attention" in n for n, ty, *_ in net.layers)
    if hd.DROPOUT in c.switches:
        masks = [net.dropout_mask(n) for n in net.dropout_layers()]
        assert masks and all(np.any(m != m.flat[0]) for m in masks)      # a mask that masks
    if hd.SPECAUG in c.switches:
        assert net.spec_augment_layers()
    if hd.IMPLICIT in c.switches:
        assert "tdnnf5" in names


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gates_under_the_mode(gpu, comm, case):
    """Repeatability of the unbound backward, then the SNAPSHOT proof and the PEER_MEAN proof with
    their early-exchange controls (dp_dev). bn-pass-through: mid-bn is the batchnorm-component of
    dp_dev.midbn_xcfg, between prefinal-l (trainable, below) and prefinal-chain (trainable, above)
    on the chain path; its step issues buckets through a wgrad of its own and records no ev_step.
    offpath: the xent branch's tensors lie above output.W in the buffer, so the plan puts them into
    the first bucket (issued after the output layer's step), not the last; whichever bucket holds
    them, their snapshot must be the zeros begin() wrote and their PEER_MEAN result 0.5 * peer."""
    rig = dd.Rig(gpu, case)
    try:
        plan = rig.plan(min_buckets=4)
        ga = dd.repeatable(rig)
        _extra_reach(rig)
        print("%s: %d buckets, %d parameters" % (case.name, len(plan), rig.P))
        dd.snapshot_proof(rig, comm, plan, ga)
        dd.peer_mean_proof(rig, comm, ga)
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# the loss scale under a communicator
# ---------------------------------------------------------------------------
LS_CASE = _CASES[0]


def _ls_state(kf, net):
    """master, fp16 weights and velocity, as bits"""
    kf.sync()
    n = net.num_params
    return dict(w32=kf.read_f32(net.master_ptr, (n,)).view(np.uint32).copy(),
                w16=kf.read_fp16(kf.nnet.nnet_weight_buffer(net.h), (n,)).view(np.uint16).copy(),
                v=kf.read_f32(kf.nnet.nnet_debug_tensor(net.h, b"vel", 0), (n,)).view(np.uint32).copy())


def _same_state(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def _ls_rig(kf):
    """tiny3c at T = 299 with row subsampling and the loss scale at its default options. The output
    gradient is 1 / 64 of history_dev.out_grad's, so that times the initial scale of 65536 it stays
    far inside fp16 on its way down the net (an objective's derivative is at most 1 per row)."""
    rig = dd.Rig(kf, LS_CASE)
    for sh in (rig.A, rig.B):
        sh.og_host = (sh.og_host.astype(np.float32) / 64).astype(np.float16)
    rig.net.set_loss_scale(True)
    return rig


def _ls_opts(kf):
    import ctypes
    o = kf.KfLossScaleOpts()
    kf.core.kf_loss_scale_default_opts(ctypes.byref(o))
    return o


def _ls_finite_peer(kf, comm, rig, optimise):
    """-> (gB, the state after the bound step). The bound step on shard A with gB as the peer's
    gradient equals the unbound update of the same state handed (gA + gB) * 0.5."""
    net, P = rig.net, rig.P
    scale = net.loss_scale_stats()["scale"]
    assert scale == _ls_opts(kf).init_scale
    ga, gb = rig.grad(rig.A, scale), rig.grad(rig.B, scale)
    rig.reach()
    for name, (b, e) in rig.ranges().items():
        assert np.isfinite(ga[b:e]).all() and np.isfinite(gb[b:e]).all() and np.any(ga[b:e]), name
    mean = ((ga + gb) * np.float32(0.5)).astype(np.float32)

    def fresh_state():
        net.set_params(rig.w0)
        net.set_loss_scale(True)
        return net.loss_scale_stats()

    st0 = fresh_state()
    kf.check(kf.core.bridge_transfer_float32(net.grad_ptr, mean.ctypes.data, P), "upload mean")
    optimise(net)
    ref, st_ref = _ls_state(kf, net), net.loss_scale_stats()
    assert np.any(ref["w32"] != dd.bits(net.flat_params(rig.w0))) and np.any(ref["v"])

    st0 = fresh_state()
    peer = kf.upload_f32(gb)
    with dd.Bound(rig, comm, comm.DEBUG_PEER_MEAN, peer.ptr):
        og = rig.forward(rig.A, scale)
        rig.fill(net.grad_ptr, 0)
        net.backward(og.ptr)
        optimise(net)               # behind kf_dp_join, no host sync between
        got = _ls_state(kf, net)
        np.testing.assert_array_equal(dd.bits(rig.read(net.grad_ptr)), dd.bits(mean))
    _same_state(got, ref, "bound step against the unbound update of the mean")
    st = net.loss_scale_stats()
    assert st == st_ref
    assert st["since"] == st0["since"] + 1 and st["scale"] == st0["scale"] and st["skipped"] == 0 and not st["last_overflow"]
    return gb, got


def test_loss_scale_finite_peer_sgd(gpu, comm):
    """nnet_sgd goes through the loss scale while it is on (update.cpp): the finite-peer case with it"""
    rig = _ls_rig(gpu)
    try:
        _ls_finite_peer(gpu, comm, rig, lambda n: n.sgd(dd.LR, dd.MOM))
    finally:
        rig.close()


def _element_in(rig, bucket):
    """a trainable element of a bucket (the check reads no alignment padding)"""
    _, b, e = bucket
    for name, (lo, hi) in rig.ranges().items():
        if max(lo, b) < min(hi, e):
            return max(lo, b)
    raise AssertionError("bucket %r holds no tensor" % (bucket,))


def test_loss_scale_peer_overflow_reaches_the_check(gpu, comm):
    """nnet_update on a bound net: a finite peer gives the unbound update of the mean; one +inf of
    the peer in the bucket issued first, one in the bucket issued last, a NaN in a middle bucket:
    each skips the step (master, fp16 weights and velocity keep their bits, the scale is multiplied
    by backoff, skipped goes up by 1): a non-finite value of another rank reaches this rank's
    decision, because kf_dp_join stands before the check. Control: with every bucket exchanged
    before the backward the producers overwrite the inf and the step is not skipped."""
    kf = gpu
    rig = _ls_rig(kf)
    try:
        net = rig.net
        plan = rig.plan(min_buckets=4)
        backoff = _ls_opts(kf).backoff
        assert 0 < backoff < 1
        gb, s1 = _ls_finite_peer(kf, comm, rig, lambda n: n.update(dd.LR, dd.MOM))

        def bound_step(bucket, value, early=False):
            poisoned = gb.copy()
            poisoned[_element_in(rig, bucket)] = value
            peer = kf.upload_f32(poisoned)
            before = net.loss_scale_stats()
            with dd.Bound(rig, comm, comm.DEBUG_PEER_MEAN, peer.ptr):
                net.dp_debug_early(early)
                og = rig.forward(rig.A, before["scale"])
                rig.fill(net.grad_ptr, 0)
                net.backward(og.ptr)
                net.update(dd.LR, dd.MOM)
                state = _ls_state(kf, net)
            return before, net.loss_scale_stats(), state

        for what, bucket, value in (("inf in the first bucket", plan[0], np.inf), ("inf in the last bucket", plan[-1], np.inf),
                                    ("NaN in a middle bucket", plan[len(plan) // 2], np.nan)):
            before, after, state = bound_step(bucket, value)
            _same_state(state, s1, what)
            assert after["skipped"] == before["skipped"] + 1 and after["last_overflow"], (what, before, after)
            assert after["scale"] == before["scale"] * backoff and after["steps"] == before["steps"] + 1, (what, before, after)
        before, after, state = bound_step(plan[0], np.inf, early=True)
        assert after["skipped"] == before["skipped"] and not after["last_overflow"], (before, after)
        assert after["scale"] == before["scale"] and after["since"] == before["since"] + 1, (before, after)
        assert np.any(state["w32"] != s1["w32"]) and np.any(state["v"] != s1["v"])
    finally:
        rig.close()


# ---------------------------------------------------------------------------
# refusals (host/modes.cpp kConflicts, the rows that name Mode::DataParallel)
# ---------------------------------------------------------------------------
def _xent_backward(rig):
    xg = rig.kf.upload_fp16(hd.out_grad(rig.case.T, seed=8))
    og = rig.forward(rig.A)
    rig.net.backward(og.ptr, xg.ptr)
    rig.kf.sync()


# (mode, config, switch on, switch off, the refusal of the switch on a bound net, the refusal of the bind)
_DP = r"on a net bound to data parallel \(nnet_bind_dp\)"
REFUSALS = {
    "self-repair": ("tiny", lambda r: r.net.set_self_repair(True), lambda r: r.net.set_self_repair(False),
                    "set_self_repair: not supported " + _DP, r"bind_dp: not supported with ReLU self-repair on \(nnet_set_self_repair\)"),
    "bn-train": ("tiny", lambda r: r.net.set_batchnorm_train(True), lambda r: r.net.set_batchnorm_train(False),
                 "set_bn_train: not supported " + _DP, r"bind_dp: not supported with training-mode BatchNorm on \(nnet_set_bn_train\)"),
    # (nnet_backward_xent is a call, not a switch: there is nothing to switch on before the bind)
    "backward-xent": ("tiny_xent", _xent_backward, None, "backward_xent: not supported " + _DP + ".*chain output's path only", None),
}
# natural gradient: tests/test_gpu_natgrad.py::test_guard_data_parallel has both orders


@pytest.mark.parametrize("mode,order", [(m, o) for m in REFUSALS for o in ("bind-first", "mode-first")
                                        if not (o == "mode-first" and REFUSALS[m][2] is None)])
def test_refusals_leave_the_net_usable(gpu, comm, mode, order):
    """each attempt raises KfError naming the other mode, and afterwards a plain bound backward gives
    the unbound gradient bits"""
    kf = gpu
    cfg, on, off, on_bound, on_bind = REFUSALS[mode]
    rig = dd.Rig(kf, Case(mode, cfg, 150))
    try:
        net = rig.net
        ga = dd.repeatable(rig)
        if order == "bind-first":
            net.bind_dp(comm, dd.BUCKET)
            with pytest.raises(kf.KfError, match=on_bound):
                on(rig)
        else:
            on(rig)
            with pytest.raises(kf.KfError, match=on_bind):
                net.bind_dp(comm, dd.BUCKET)
            off(rig)
            net.bind_dp(comm, dd.BUCKET)
        n0 = comm.stats()[0]
        g = rig.grad(rig.A)
        assert comm.stats()[0] - n0 == len(net.dp_plan(dd.BUCKET))
        np.testing.assert_array_equal(dd.bits(g), dd.bits(ga))
    finally:
        kf.sync()
        rig.net.bind_dp(None, 0)
        rig.close()
