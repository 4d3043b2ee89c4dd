"""Training the xent branch: nnet_backward_xent, the backward with two seeds, and
EgsTrainer with TrainConfig.xent_regularize, on configs/tiny_xent.xconfig.

Reference of the two-seed backward: the CPU oracle's orc_net_backward_top called twice on one
forward (the GPU's ReLU decisions replayed), seeded at output-xent and at the chain output, the
two results added in float64. The oracle rounds every stored output gradient to fp16 in each
walk, the GPU rounds the branch's gradient at the branch point once (gx) and the sum once
(g = rne(acc + gx)): a difference of fp16 roundings, inside the project's 5e-3 rel-Frobenius bar
for gradients. Both seeds are N(0, 0.05^2) fp16: on the CPU oracle the chain-only
gradient of every parameter from the branch point down then lies 0.62 .. 0.80 (rel-Frobenius)
from the sum, far above 10 x the bar.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import xent_ref as xr_
from conftest import rel_fro

pytestmark = pytest.mark.gpu

BAR = 5e-3
BRANCH = ("prefinal-xent.", "output-xent.")
CHAIN_ONLY = ("prefinal-chain.", "output.")
P = 200


def _seeds(T, rows=None):
    """fp16 seeds [T x P] of the chain output and of output-xent; rows: non-zero on these only"""
    og = (np.random.default_rng(7).standard_normal((T, P)) * 0.05).astype(np.float16)
    xg = (np.random.default_rng(8).standard_normal((T, P)) * 0.05).astype(np.float16)
    if rows is not None:
        keep = np.zeros(T, bool)
        keep[rows] = True
        og[~keep] = 0
        xg[~keep] = 0
    return og, xg


def _net(kf, T, xconfig="tiny_xent.xconfig"):
    from kfp16 import synth
    xcfg = synth.load_xconfig(xconfig)
    net = kf.Network(xcfg, max_frames=T)
    params, bns = synth.init_network(net)
    feats = synth.make_features(T, 40)
    fb = kf.upload_fp16(feats)
    return net, xcfg, params, bns, feats, fb


@pytest.mark.parametrize("T", [150, 333])
def test_two_seed_backward_matches_oracle_sum(gpu, T):
    kf = gpu
    from kfp16 import synth
    net, xcfg, params, bns, feats, fb = _net(kf, T)
    net.forward(fb.ptr, T)
    og, xg = _seeds(T)
    gb, xb = kf.upload_fp16(og), kf.upload_fp16(xg)
    net.backward(gb.ptr, xb.ptr)
    got = net.read_grads()
    tp = {k: synth.trunc_fp16(v) for k, v in params.items()}
    on = oracle.OracleNet(xcfg, tp, bns, round_mode=oracle.ROUND_FUSED, threads=16)
    on.forward(feats.astype(np.float32), force_masks=net.relu_masks())
    L = oracle.lib()
    # the xent walk first, on the fresh oracle: the chain-only layers have no gradient yet (zeros)
    g32 = np.ascontiguousarray(xg, np.float32)
    assert L.orc_net_backward_top(C.byref(on.net), on.x.ctypes.data, g32.ctypes.data, on.index["output-xent"]) == 0
    xent = on.grads()
    g32 = np.ascontiguousarray(og, np.float32)
    assert L.orc_net_backward_top(C.byref(on.net), on.x.ctypes.data, g32.ctypes.data, on.chain_output()) == 0
    chain = on.grads()
    on.close()
    for k in chain:
        if k.startswith(BRANCH):          # (still the xent walk's: the chain walk does not visit them)
            chain[k] = np.zeros_like(chain[k])
        if k.startswith(CHAIN_ONLY):
            assert not np.any(xent[k]), k
    errs = {}
    for k in chain:
        ref = chain[k].astype(np.float64) + xent[k].astype(np.float64)
        errs[k] = rel_fro(got[k], ref)
        if k.startswith(BRANCH):
            assert np.any(got[k]), k
        elif not k.startswith(CHAIN_ONLY):
            # from the branch point down: the chain-only gradient is not the answer
            assert rel_fro(chain[k], ref) >= 10 * BAR, (k, rel_fro(chain[k], ref))
    print("T=%d: largest rel-Frobenius error %.2e (%s)" % (T, max(errs.values()), max(errs, key=errs.get)))
    bad = {k: v for k, v in errs.items() if v > BAR}
    assert not bad, bad
    net.close()


def test_chain_only_backward_after_a_two_seed_one(gpu):
    """nnet_backward after nnet_backward_xent: bit-identical to one on a fresh net, the branch
    exactly zero again; and the two-seed backward itself replays bit for bit."""
    kf = gpu
    T = 150
    og, xg = _seeds(T)
    gb, xb = kf.upload_fp16(og), kf.upload_fp16(xg)
    fresh, *_, fb = _net(kf, T)
    fresh.forward(fb.ptr, T)
    fresh.backward(gb.ptr)
    want = fresh.read_grads()
    fresh.close()
    net, *_ = _net(kf, T)
    net.forward(fb.ptr, T)
    net.backward(gb.ptr, xb.ptr)
    two = net.read_grads()
    net.backward(gb.ptr, xb.ptr)
    again = net.read_grads()
    net.backward(gb.ptr)
    got = net.read_grads()
    for k in want:
        np.testing.assert_array_equal(two[k].view(np.uint32), again[k].view(np.uint32), err_msg=k)
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
        if k.startswith(BRANCH):
            assert np.any(two[k]) and not np.any(got[k]), k
    net.close()


def test_two_seed_backward_on_the_row_set(gpu):
    """Row subsampling: both seeds in compact rows (placed by nnet_row_set) against both in full
    rows, non-zero on the supervised rows only; every gradient within the bar
    tests/test_gpu_row_subsampling.py holds compact rows to against all rows (rel-Frobenius 1e-5)."""
    kf = gpu
    T = 333
    sup = np.arange(30, T, 3)
    og, xg = _seeds(T, sup)
    res = {}
    for sub in (False, True):
        net, *_, fb = _net(kf, T)
        if sub:
            net.set_row_subsampling(3)
        net.forward(fb.ptr, T)
        tc, tc0, rows = net.row_set()
        assert (tc > 0) == sub
        a, b = (og[rows], xg[rows]) if sub else (og, xg)
        gb, xb = kf.upload_fp16(a), kf.upload_fp16(b)
        net.backward(gb.ptr, xb.ptr)
        res[sub] = net.read_grads()
        net.close()
    worst = 0.0
    for k, v in res[False].items():
        assert np.any(v), k
        worst = max(worst, rel_fro(res[True][k], v))
        assert rel_fro(res[True][k], v) <= 1e-5, (k, rel_fro(res[True][k], v))
    print("compact rows against all rows: largest rel-Frobenius difference %.2e" % worst)


def test_two_seed_backward_refusals(gpu):
    """MXFP8 mode, a net bound to data parallel, a net without output-xent: each an error whose
    text names the cause (most of this test's time is the one-rank communicator)."""
    kf = gpu
    from kfp16 import dp
    T = 150
    og, xg = _seeds(T)
    gb, xb = kf.upload_fp16(og), kf.upload_fp16(xg)
    net, *_, fb = _net(kf, T)
    net.set_fp8(True)
    net.forward(fb.ptr, T)
    with pytest.raises(kf.KfError, match="nnet_set_fp8"):
        net.backward(gb.ptr, xb.ptr)
    net.set_fp8(False)
    comm = dp.Communicator(0, 1, dp.unique_id(), 0)
    net.bind_dp(comm, 1 << 20)
    net.forward(fb.ptr, T)
    with pytest.raises(kf.KfError, match="nnet_bind_dp.*chain output's path only"):
        net.backward(gb.ptr, xb.ptr)
    net.bind_dp(None, 0)
    net.backward(gb.ptr, xb.ptr)          # neither mode left a trace
    assert np.any(net.read_grads()["output-xent.W"])
    comm.close()
    net.close()
    plain, *_ = _net(kf, T, "tiny.xconfig")
    plain.forward(fb.ptr, T)
    with pytest.raises(kf.KfError, match="no output-xent layer"):
        plain.backward(gb.ptr, xb.ptr)
    plain.close()


# ---------------------------------------------------------------- the trainer
def _egs(tmp_path, n=4):
    import egs_writer as W
    from kfp16 import egs, synth
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, n, rows=(150, 183, 129), num_pdfs=P, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=n).next_batch()
    return batch, synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=P)


XENT_COMPS = ("prefinal-xent.affine", "prefinal-xent.linear", "output-xent.affine")
XR = 0.1


def _factor(net):
    """the recipes' learning-rate factor 0.5 / xent_regularize on the xent components"""
    for c in net.components():
        if c["name"] in XENT_COMPS:
            net.set_component_opts(c["name"], c["max_change"], c["l2"], 0.5 / XR)
    assert sorted(c["name"] for c in net.components() if c["lr_factor"] == 5.0) == sorted(XENT_COMPS)


def test_trainer_with_xent_regularize(gpu, tmp_path):
    """Three EgsTrainer steps with xent_regularize = 0.1, the Kaldi update, the learning-rate
    factor on the xent components, NG-SGD and training-mode BatchNorm together: everything finite,
    the parameters bit-identical to the same steps composed by hand from Chain.compute, Chain.xent,
    Network.backward(.., xent) and update. The first step's xent objective per frame lies within
    0.5 of -log P: with the TDNN-F BatchNorms normalising the minibatch, synth.init_network's
    output-xent is near uniform (measured -5.43 against -5.30). On the CPU oracle, which has the
    frozen synthetic statistics only, it is not (max |y + log P| = 4.3, objective per frame
    -12.7), so the window could not be confirmed there; the objective is therefore also held to
    the float64 reference (tests/xent_ref.py) on the step's own activations, 1e-3 per frame."""
    kf = gpu
    from kfp16 import chain, synth, trainer
    batch, den = _egs(tmp_path)
    xcfg = synth.load_xconfig("tiny_xent.xconfig")
    cfg = trainer.TrainConfig(learning_rate=1e-3, momentum=0.9, kaldi_update=True, max_param_change=1.0,
                              natural_gradient=True, batchnorm_train=True, xent_regularize=XR)
    tr = trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=800, config=cfg)
    synth.init_network(tr.net)
    _factor(tr.net)
    T = batch.total_frames
    row0, frames = trainer.chain_rows(batch.frame_offsets, batch.num_frames, batch.frames_per_seq, 3, 30)
    objs = []
    for step in range(3):
        tr.step(batch)
        r = tr.result()
        assert r.num_ok == batch.batch_size and np.isfinite(r.objf) and np.isfinite(r.xent_objf)
        assert r.xent_weight == r.total_weight == float(frames.sum())
        objs.append(r.xent_objf / r.xent_weight)
        if step == 0:
            x = tr.net.read_activation("output")
            y = tr.net.read_activation("output-xent")
            ref = 0.0
            for i, f in enumerate(batch.num_fsts()):
                rows = row0[i] + np.arange(frames[i]) * 3
                ref += xr_.xent_f64(f, x[rows], y[rows], XR, 1.0)[1]
            print("first step: xent objective per frame %.4f (float64 %.4f), -log P %.4f" % (
                objs[0], ref / frames.sum(), -np.log(P)))
            assert abs(r.xent_objf - ref) / frames.sum() <= 1e-3, (r.xent_objf, ref)
            assert abs(objs[0] + np.log(P)) <= 0.5, objs[0]
            assert np.any(kf.read_fp16(tr.xent_grad.ptr, (T, P))[row0[0]])
    got = tr.net.get_params()
    assert all(np.all(np.isfinite(v)) for v in got.values())
    # by hand
    net = kf.Network(xcfg, max_frames=800)
    net.set_natural_gradient(True)
    net.set_batchnorm_train(True)
    net.batchnorm_zero_stats()
    synth.init_network(net)
    _factor(net)
    feat = kf.DeviceBuffer(800 * 40 * 2)
    g, xg = kf.DeviceBuffer(800 * P * 2), kf.DeviceBuffer(800 * P * 2)
    dg = chain.DenGraph(den)
    obj = chain.Chain(dg, max_seqs=8, max_frames=800 // 3 + 1)
    o = chain.KfChainOpts.default()
    opts = chain.KfChainOpts(o.l2_regularize, o.out_of_range_regularize, o.leaky_hmm_coefficient, XR, o.supervision_weight)
    for step in range(3):
        batch.features_to_device(feat.ptr, 40)
        kf.core.bridge_gpu_memset(g.ptr, 0, T * P * 2)
        kf.core.bridge_gpu_memset(xg.ptr, 0, T * P * 2)
        net.forward(feat.ptr, T)
        nb = chain.NumBatch(batch.num_fsts())
        obj.compute(nb, net.activation("output")[0], P, T, row0, frames, 3, g.ptr, P, opts)
        obj.xent(nb, net.activation("output-xent")[0], P, xg.ptr, P, opts)
        net.backward(g.ptr, xg.ptr)
        net.update(1e-3, 0.9, 1.0, float(frames.sum()))
        kf.sync()
        xo, xw = obj.xent_result()
        assert xo / xw == objs[step]
    want = net.get_params()
    for k in want:
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
    # the branch trains: its parameters moved
    start, _ = synth.init_network(net)
    assert all(np.any(got[k] != synth.trunc_fp16(start[k])) for k in got if k.startswith(BRANCH))
    net.close()


def test_trainer_without_xent_regularize_is_unchanged(gpu, tmp_path):
    """xent_regularize = 0: three steps bit-identical to a trainer built without the field, the
    result without the xent attributes, the branch left where it started."""
    kf = gpu
    from kfp16 import synth, trainer
    batch, den = _egs(tmp_path)
    xcfg = synth.load_xconfig("tiny_xent.xconfig")
    out = []
    for kw in (dict(), dict(xent_regularize=0.0)):
        cfg = trainer.TrainConfig(learning_rate=1e-3, momentum=0.9, kaldi_update=True, max_param_change=1.0, **kw)
        tr = trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=800, config=cfg)
        start, _ = synth.init_network(tr.net)
        assert tr.xent_grad is None
        for _ in range(3):
            tr.step(batch)
        r = tr.result()
        assert not hasattr(r, "xent_objf")
        out.append((tr.net.get_params(), r.objf))
        tr.net.close()
    assert out[0][1] == out[1][1]
    for k, v in out[0][0].items():
        np.testing.assert_array_equal(v.view(np.uint32), out[1][0][k].view(np.uint32), err_msg=k)
        if k.startswith(BRANCH):
            np.testing.assert_array_equal(v, synth.trunc_fp16(start[k]), err_msg=k)
