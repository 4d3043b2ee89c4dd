"""The reference of the conv / prefinal / batchnorm-component training-mode BatchNorm
(tests/bn_sites_ref.py) checked without a device: the block rule against torch
float64 autograd, the numpy prefinal-layer in frozen mode against the committed oracle, the
separation of the train-mode reference from the frozen computation on the seeds the GPU tests
use, and the host layer's site selector on a layout-only network."""
import numpy as np
import pytest

import bn_sites_ref as bs
from conftest import rel_fro

T = 300
SEQ = [0, 90, 200, 300]


# ---------------------------------------------------------------------------
# the block rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("rows,H,F", [(7, 2, 8), (50, 10, 16)])
def test_block_rule_against_torch(rows, H, F, with_mask):
    import torch
    rng = np.random.default_rng(rows + H + F)
    eps, rms = 1e-3, 0.75
    z = rng.standard_normal((rows, H * F))
    bits = (z > -0.3) if with_mask else np.ones_like(z, bool)
    r = np.where(bits, z + 0.3, 0.0) if with_mask else z
    G = rng.standard_normal((rows, H * F))
    f = bs.bn_block_forward(r, H, F, eps, rms)
    a, b, gr = bs.bn_block_backward(G, r, H, F, f["scale"], f["shift"], rms, bits if with_mask else None)

    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    rt = torch.relu(zt + 0.3) if with_mask else zt
    # [rows, H F] -> [rows, F, H]: batch_norm's channel axis is the block
    y = torch.nn.functional.batch_norm(rt.reshape(rows, H, F).permute(0, 2, 1), None, None, training=True, eps=eps) * rms
    y = y.permute(0, 2, 1).reshape(rows, H * F)
    (y * torch.tensor(G)).sum().backward()
    assert np.max(np.abs(f["out"] - y.detach().numpy())) <= 1e-10
    rv = r.reshape(rows * H, F)
    assert np.max(np.abs(f["mean"] - rv.mean(0))) <= 1e-10 and np.max(np.abs(f["var"] - rv.var(0))) <= 1e-10
    assert np.max(np.abs(gr - zt.grad.numpy())) <= 1e-10
    # a, b as the rule states them
    Gv, yhat = G.reshape(rows * H, F), (f["out"] / rms).reshape(rows * H, F)
    assert np.max(np.abs(a - Gv.mean(0))) <= 1e-10 and np.max(np.abs(b - (Gv * yhat).mean(0))) <= 1e-10


# ---------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------
def _setup(cfg, sites=None):
    """the synthetic parameters of synth.init_network and, with `sites` governed, the frozen
    statistics tests/test_gpu_bn_sites.py uses for that case (bn_sites_ref.matched_bns), without a
    device; sites None: init_network's random statistics everywhere"""
    import kfp16
    from kfp16 import synth
    xcfg = synth.load_xconfig(cfg)
    net = kfp16.Network(xcfg, max_frames=T, layout_only=True)
    params = synth.make_params(net.params, seed=42)
    conv_fout, prefinal = synth.layer_dims(net)
    bns = synth.make_bn_all(synth.bn_specs(net.layers, conv_fout, prefinal))
    tp = {k: synth.trunc_fp16(v) for k, v in params.items()}
    feats = synth.make_features(T, 40, seed=1234).astype(np.float32)
    og = (np.random.default_rng(7).standard_normal((T, 200)) * 0.05).astype(np.float16).astype(np.float32)
    iv = None
    if "ivec" in cfg:
        iv = (np.random.default_rng(T).standard_normal((3, 100)) * 2).astype(np.float16).astype(np.float32)
    net.close()
    if sites is not None:
        bns = bs.matched_bns(xcfg, tp, bns, feats, sites, iv, np.asarray(SEQ, np.int32) if iv is not None else None)
    return xcfg, tp, bns, feats, og, iv


def test_prefinal_restatement_against_oracle_frozen():
    """the numpy prefinal-layer with frozen BatchNorms is the oracle's, within fp16 rounding: its
    four rounding points forward, four backward, 2^-11 relative each"""
    import oracle
    xcfg, tp, bns, feats, og, _ = _setup("tiny.xconfig")
    on = oracle.OracleNet(xcfg, tp, bns, round_mode=oracle.ROUND_FUSED, threads=8)
    on.forward(feats)
    x = on.act("prefinal-l")
    n = "prefinal-chain"
    f = bs.prefinal_forward(x, tp[n + ".BigW"], tp[n + ".BigBias"].reshape(-1), tp[n + ".SmallW"], bns[(n, 0)], bns[(n, 1)],
                            force_mask=on.mask(n))
    bound = 4 * 2.0 ** -11
    assert rel_fro(f["act"], on.act(n)) <= bound, rel_fro(f["act"], on.act(n))
    on.backward(og)
    ref = on.grads()
    gout = np.ctypeslib.as_array(on.net.gact[on.index[n]], shape=(T * 64,)).reshape(T, 64)
    gW, gb, gW2, gin = bs.prefinal_backward(gout, f)
    gpl = np.ctypeslib.as_array(on.net.gact[on.index["prefinal-l"]], shape=(T * 64,)).reshape(T, 64)
    for got, want, what in ((gW, ref[n + ".BigW"], "BigW"), (gb.reshape(1, -1), ref[n + ".BigBias"], "BigBias"),
                            (gW2, ref[n + ".SmallW"], "SmallW"), (gin, gpl, "input gradient")):
        print("%s: %.2e" % (what, rel_fro(got, want)))
        assert rel_fro(got, want) <= bound, what
    on.close()


def _train_and_frozen(cfg, sites):
    """On the inputs of the GPU case (cfg, sites): the train-mode reference, the plain oracle fed
    its batch statistics with the same ReLU decisions, and the plain oracle at the case's own frozen
    statistics. -> (train acts, train grads, frozen-fed acts, frozen-fed grads, frozen acts, the
    governed layers)"""
    import oracle
    xcfg, tp, bns, feats, og, iv = _setup(cfg, sites)
    kw = dict(ivectors=iv, seq_off=np.asarray(SEQ, np.int32)) if iv is not None else {}
    ref = bs.BnSitesOracle(xcfg, tp, bns, sites, threads=8)
    ref.forward(feats, **kw)
    # the conditioning of the comparison from the features (BnSitesOracle.amplification): an error
    # of 1e-3 at a governed stage's input, half of the activations' bound, stays inside that bound
    amp = ref.amplification()
    print("amplification of an input error per governed stage: " + ", ".join("%s=%.2f" % kv for kv in amp.items()))
    assert all(a <= 2.0 for a in amp.values()), amp
    grads = ref.backward(og)
    acts, masks = dict(ref.acts), dict(ref.masks)
    governed = sorted({name for name, _ in ref.stats})
    b2 = dict(bns)
    for (name, which), (m, v) in ref.stats.items():
        d = m.size
        b2[(name, which)] = (m.astype(np.float32), v.astype(np.float32), np.ones(d, np.float32), np.zeros(d, np.float32))
    ref.close()
    on = oracle.OracleNet(xcfg, tp, b2, round_mode=oracle.ROUND_FUSED, threads=8)
    on.forward(feats, force_masks=masks, **kw)
    facts = {n: on.act(n) for n in acts}
    on.backward(og)
    fgrads = on.grads()
    on.close()
    on = oracle.OracleNet(xcfg, tp, bns, round_mode=oracle.ROUND_FUSED, threads=8)
    on.forward(feats, **kw)
    iacts = {n: on.act(n) for n in acts}
    on.close()
    return acts, grads, facts, fgrads, iacts, governed


# The separation, on exactly the inputs of each case of tests/test_gpu_bn_sites.py, so that a pass
# there is a pass of the feature and not of the frozen path:
# - backward: the frozen computation fed the batch statistics lies at least 10 x the GPU
#   comparison's gradient tolerance (5e-3) from the train-mode reference on a weight gradient of a
#   governed layer;
# - forward: the frozen forward at the case's own frozen statistics (what a forward that took the
#   statistics and then applied the frozen pair would give) lies at least 5e-2, 25 x the
#   activations' tolerance, from the reference on the output of every governed layer.
# (kind, config, sites, the gradients that must differ)
ALL = ["tdnnf", "conv", "prefinal", "batchnorm"]
SEPARATION = [
    ("all", "tiny.xconfig", ALL, ["cnn1.W", "cnn4.W", "tdnnf5.AffineW", "prefinal-chain.BigW"]),
    ("all ivector", "tiny_ivec.xconfig", ALL, ["cnn1.W", "ivector-linear.W", "prefinal-chain.BigW"]),
    ("conv", "tiny.xconfig", ["conv"], ["cnn1.W", "cnn2.W", "cnn3.W", "cnn4.W"]),
    ("conv small-fin", "tiny_ivec.xconfig", ["conv"], ["cnn1.W", "cnn2.W"]),
    ("prefinal", "tiny.xconfig", ["prefinal"], ["prefinal-chain.BigW"]),
    ("ivector-batchnorm", "tiny_ivec.xconfig", ["batchnorm"], ["ivector-linear.W"]),
]


def test_random_frozen_statistics_are_ill_conditioned():
    """why the network tests do not use synth.init_network's random statistics: a governed
    prefinal-layer above layers frozen at them amplifies an input error more than three times"""
    xcfg, tp, bns, feats, og, _ = _setup("tiny.xconfig")
    ref = bs.BnSitesOracle(xcfg, tp, bns, ["prefinal"], threads=8)
    ref.forward(feats)
    amp = ref.amplification()
    ref.close()
    print("random statistics: %.2f" % amp["prefinal-chain"])
    assert amp["prefinal-chain"] > 3.0


@pytest.mark.parametrize("kind,cfg,sites,keys", SEPARATION, ids=[s[0] for s in SEPARATION])
def test_separation_from_the_frozen_computation(kind, cfg, sites, keys):
    acts, grads, facts, fgrads, iacts, governed = _train_and_frozen(cfg, sites)
    # (the forward is the frozen forward fed the batch statistics, up to the fp16 rounding of r,
    # which the layers above carry on: printed, not a condition)
    print("%s: forward against the frozen forward fed the batch statistics, largest %.2e" % (
        kind, max(rel_fro(acts[n], facts[n]) for n in acts)))
    fsep = {n: rel_fro(iacts[n], acts[n]) for n in governed}
    print("%s: frozen forward at the case's own statistics differs by %s" % (kind, ", ".join("%s=%.2e" % kv for kv in fsep.items())))
    assert all(v >= 5e-2 for v in fsep.values()), fsep
    for k in keys:
        sep = rel_fro(fgrads[k], grads[k])
        print("%s: frozen-statistics gradient of %s differs by %.3e" % (kind, k, sep))
        assert sep >= 5e-2, (k, sep)
    # a gradient above every governed layer does not depend on how they differentiate
    assert rel_fro(fgrads["output.W"], grads["output.W"]) <= 5e-3


def test_separation_idct_batchnorm():
    """idct-batchnorm has nothing trainable below it: training mode shows in its output alone,
    against the output under the initial (frozen) statistics"""
    acts, grads, facts, fgrads, iacts, governed = _train_and_frozen("tiny.xconfig", ["batchnorm"])
    assert governed == ["idct-batchnorm"]
    sep = rel_fro(iacts["idct-batchnorm"], acts["idct-batchnorm"])
    print("idct-batchnorm: output under the initial statistics differs by %.3e" % sep)
    assert sep >= 5e-2
    assert rel_fro(facts["idct-batchnorm"], acts["idct-batchnorm"]) <= 2e-3
    # what the normalisation promises: column mean 0, mean square var / (var + eps)
    y = acts["idct-batchnorm"].astype(np.float64)
    assert np.abs(y.mean(0)).max() <= 2.0 ** -9
    for k in grads:
        assert rel_fro(fgrads[k], grads[k]) <= 5e-3, k


def test_component_restatement():
    """the numpy batchnorm-component against the oracle's frozen one fed the same statistics"""
    import oracle
    xcfg, tp, bns, feats, og, iv = _setup("tiny_ivec.xconfig", ["batchnorm"])
    r = bs.f16(iv.astype(np.float64) @ tp["ivector-linear.W"].astype(np.float64))
    (m, v), out = bs.component_stats(r, 0.025)
    b2 = dict(bns)
    b2[("ivector-batchnorm", 0)] = (m.astype(np.float32), v.astype(np.float32), np.ones(200, np.float32), np.zeros(200, np.float32))
    on = oracle.OracleNet(xcfg, tp, b2, round_mode=oracle.ROUND_FUSED, threads=8)
    on.forward(feats, ivectors=iv, seq_off=np.asarray(SEQ, np.int32))
    assert rel_fro(out, on.act("ivector-batchnorm")) <= 2 * 2.0 ** -11
    on.close()
    assert abs(np.sqrt((out * out).mean()) - 0.025) <= 0.005   # target-rms, up to eps and B = 3


# ---------------------------------------------------------------------------
# the site selector on a layout-only network
# ---------------------------------------------------------------------------
def test_site_selector_layout():
    import kfp16
    from kfp16 import synth
    net = kfp16.Network(synth.load_xconfig("tiny_xent.xconfig"), max_frames=64, layout_only=True)
    tdnnf = ["tdnnf3", "tdnnf4"]
    assert net.batchnorm_train_sites() == 1 and net.batchnorm_train_layers() == tdnnf
    net.set_batchnorm_train_sites("conv")
    assert net.batchnorm_train_sites() == 2 and net.batchnorm_train_layers() == ["cnn1", "cnn2"]
    net.set_batchnorm_train_sites(["prefinal", "batchnorm"])
    assert net.batchnorm_train_layers() == ["idct-batchnorm", "prefinal-chain", "prefinal-xent"]
    net.set_batchnorm_train_sites("all")
    assert net.batchnorm_train_sites() == 15
    assert net.batchnorm_train_layers() == ["idct-batchnorm", "cnn1", "cnn2"] + tdnnf + ["prefinal-chain", "prefinal-xent"]
    net.set_batchnorm_train_sites("tdnnf,conv")
    assert net.batchnorm_train_sites() == 3
    assert kfp16.nnet.nnet_bn_dim(net.h, b"cnn2", 0) == 32
    assert kfp16.nnet.nnet_bn_dim(net.h, b"prefinal-chain", 0) == 256 and kfp16.nnet.nnet_bn_dim(net.h, b"prefinal-chain", 1) == 64
    assert kfp16.nnet.nnet_bn_dim(net.h, b"tdnnf3", 0) == 256 and kfp16.nnet.nnet_bn_dim(net.h, b"idct-batchnorm", 0) == 40
    assert kfp16.nnet.nnet_bn_dim(net.h, b"tdnnf3", 1) < 0 and kfp16.nnet.nnet_bn_dim(net.h, b"prefinal-l", 0) < 0
    with pytest.raises(kfp16.KfError, match="KF_BN_SITE"):
        net.set_batchnorm_train_sites(16)
    with pytest.raises(kfp16.KfError, match="unknown site"):
        net.set_batchnorm_train_sites("convolution")
    net.set_batchnorm_train_sites(1)
    assert net.batchnorm_train_layers() == tdnnf
    net.close()
