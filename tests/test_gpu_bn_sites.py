"""Training-mode BatchNorm on the conv, prefinal and batchnorm-component sites (kf_nnet.h
nnet_set_bn_train_sites): the network on configs/tiny.xconfig (a conv with one input
filter, a strided conv above a governed conv, prefinal, idct-batchnorm), tiny_ivec.xconfig (the
small-fin conv, ivector-batchnorm over 3 sequences) and tiny_xent.xconfig (prefinal-xent), 300
frames, against the staged reference (tests/bn_sites_ref.py) with the GPU's ReLU decisions
replayed. Tolerances are test_gpu_nnet.py's and test_gpu_bn_train.py's for the same tensors:
activations 2e-3 relative Frobenius and 1e-2 of the largest value, batch statistics 2e-3,
gradients 5e-3. The layers a comparison leaves frozen carry statistics that match the data
(bn_sites_ref.matched_bns), as a trained model's do; the governed BatchNorms keep
synth.init_network's random frozen statistics, and with every site governed, or the
batchnorm-components alone, nothing is matched. tests/test_bn_sites_ref.py asserts, without a
device and on exactly these inputs, that the frozen forward at those statistics lies >= 5e-2 from
the reference on every governed layer's output, that the frozen computation fed the batch
statistics lies >= 5e-2 from it on a governed layer's weight gradient, and that no governed stage
amplifies an error of its input more than twice (with the layers below a governed prefinal-layer
frozen at random statistics the stage does, 3.6 times)."""
import numpy as np
import pytest

import bn_sites_ref as bs
from conftest import max_abs_rel, rel_fro

pytestmark = pytest.mark.gpu

T = 300
SEQ = np.asarray([0, 90, 200, 300], np.int32)
ALL = ["tdnnf", "conv", "prefinal", "batchnorm"]
CASES = [("tiny.xconfig", ["conv"]), ("tiny.xconfig", ["prefinal"]), ("tiny.xconfig", ["batchnorm"]), ("tiny.xconfig", ALL),
         ("tiny_ivec.xconfig", ["conv"]), ("tiny_ivec.xconfig", ["batchnorm"]), ("tiny_ivec.xconfig", ALL)]
PER_SEQ = {"ivector-linear", "ivector-batchnorm"}


def _features(seed=1234, frames=T):
    from kfp16 import synth
    return synth.make_features(frames, 40, seed=seed)


def _out_grad(frames=T, seed=7):
    return (np.random.default_rng(seed).standard_normal((frames, 200)) * 0.05).astype(np.float16)


def _ivectors(B=3, seed=T):
    return (np.random.default_rng(seed).standard_normal((B, 100)) * 2).astype(np.float16)


MATCHED = {}   # (config, sites) -> the frozen statistics of the case, computed once


class Net:
    """a network on its synthetic parameters, with its inputs on the device"""

    def __init__(self, kf, cfg, xcfg=None, frames=T, seq=SEQ, matched=None):
        """matched: the sites a reference comparison will govern. The layers that stay frozen then
        carry statistics that match the data (bn_sites_ref.matched_bns: under synth.init_network's
        random ones the comparison from the features is ill-conditioned); the governed ones keep
        the random statistics, far from the batch's. None: init_network's everywhere."""
        from kfp16 import synth
        self.kf, self.frames, self.seq = kf, frames, seq
        self.xcfg = xcfg or synth.load_xconfig(cfg)
        self.net = kf.Network(self.xcfg, max_frames=T)
        self.params, self.bns = synth.init_network(self.net)
        self.feats, self.og = _features(frames=frames), _out_grad(frames)
        self.ivec = _ivectors(len(seq) - 1) if "ivector" in self.xcfg else None
        if matched is not None:
            key = (cfg, tuple(matched))
            if key not in MATCHED:
                tp = {k: synth.trunc_fp16(v) for k, v in self.params.items()}
                MATCHED[key] = bs.matched_bns(self.xcfg, tp, self.bns, self.feats.astype(np.float32), matched, threads=16,
                                              **self.oracle_kw())
            self.bns = MATCHED[key]
            for (name, which), (m, v, g, b) in self.bns.items():
                self.net.set_bn(name, which, m, v, g, b, eps=1e-3)
        self.fb, self.gb = kf.upload_fp16(self.feats), kf.upload_fp16(self.og)
        self.ib = kf.upload_fp16(self.ivec) if self.ivec is not None else None

    def forward(self):
        if self.ib is not None:
            self.net.forward_ivector(self.fb.ptr, self.frames, self.ib.ptr, self.seq)
        else:
            self.net.forward(self.fb.ptr, self.frames)

    def acts(self):
        B = len(self.seq) - 1
        return {n: self.net.read_activation(n)[:B if n in PER_SEQ else None].copy() for n, *_ in self.net.layers}

    def run(self):
        self.forward()
        acts = self.acts()
        self.net.backward(self.gb.ptr)
        return acts, self.net.read_grads()

    def governed_stats(self):
        out = {}
        for n in self.net.batchnorm_train_layers():
            out[(n, 0)] = self.net.batchnorm_batch_stats(n, 0)
            if n.startswith("prefinal"):
                out[(n, 1)] = self.net.batchnorm_batch_stats(n, 1)
        return out

    def oracle_kw(self):
        return dict(ivectors=self.ivec.astype(np.float32), seq_off=self.seq) if self.ivec is not None else {}

    def close(self):
        self.net.close()


def _stat_errors(key, got, want):
    """errors of a BatchNorm's batch (mean, var) against the reference's, each to be <= 2e-3:
    relative Frobenius, test_gpu_bn_train.py's measure, with one exception"""
    (m, v), (mr, vr) = got, want
    em, ev = rel_fro(m, mr), rel_fro(v, vr)
    if key[1] == 1:
        # The exception: a prefinal layer's BatchNorm 1 sees aux W, and aux has column mean 0
        # (BatchNorm 0 made it so). Its mean is rounding noise around 0, 1e-4 of a column's rms, and
        # has no relative error to speak of. The bound there is absolute and per column:
        # |mean - ref| <= 2e-3 rms of the column, rms^2 = var + mean^2 (the largest ratio is returned).
        em = float(np.max(np.abs(m - mr) / np.sqrt(vr + mr * mr)))
    return em, ev


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# each kind alone, then all of them, against the staged reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,sites", CASES, ids=["%s-%s" % (c.split(".")[0], "all" if s is ALL else s[0]) for c, s in CASES])
def test_sites_against_reference(gpu, cfg, sites):
    import oracle  # noqa: F401  (BnSitesOracle imports it)
    from kfp16 import synth
    kf = gpu
    n = Net(kf, cfg, matched=sites)
    n.net.set_batchnorm_train_sites(sites)
    assert n.net.batchnorm_train_sites() == kf.bn_sites_mask(sites)
    n.net.set_batchnorm_train(True)
    n.forward()
    acts, stats, relu = n.acts(), n.governed_stats(), n.net.relu_masks()
    n.net.backward(n.gb.ptr)
    grads = n.net.read_grads()
    tp = {k: synth.trunc_fp16(v) for k, v in n.params.items()}
    ref = bs.BnSitesOracle(n.xcfg, tp, n.bns, sites, threads=16)
    ref.forward(n.feats.astype(np.float32), **n.oracle_kw())
    assert set(k for k in ref.stats) == set(stats), (sorted(ref.stats), sorted(stats))
    worst = 0.0
    for name, want in ref.acts.items():
        got = acts[name].astype(np.float32)
        e, m = rel_fro(got, want), max_abs_rel(got, want)
        worst = max(worst, e / 2e-3, m / 1e-2)
        assert e <= 2e-3 and m <= 1e-2, (name, e, m)
    for key, (mr, vr) in ref.stats.items():
        em, ev = _stat_errors(key, stats[key], (mr, vr))
        worst = max(worst, em / 2e-3, ev / 2e-3)
        assert em <= 2e-3 and ev <= 2e-3, (key, em, ev)
    ref.forward(n.feats.astype(np.float32), force_masks=relu, **n.oracle_kw())
    want = ref.backward(n.og.astype(np.float32))
    ref.close()
    errs = {k: rel_fro(grads[k], want[k]) for k in want}
    print("worst forward error / tolerance %.2f; grad errors: %s" % (worst, ", ".join(f"{k}={v:.2e}" for k, v in errs.items())))
    assert set(errs) == set(grads)
    bad = {k: v for k, v in errs.items() if v > 5e-3}
    assert not bad, bad
    n.close()


def test_prefinal_xent_branch(gpu):
    """nnet_backward_xent with both prefinal layers governed: each branch from the GPU's own
    activation at the branch point (prefinal-l) in numpy float64, the two input gradients added
    there; the gradients of both branches' parameters and of the branch point's weight"""
    from kfp16 import synth
    kf = gpu
    n = Net(kf, "tiny_xent.xconfig")
    n.net.set_batchnorm_train_sites("prefinal")
    assert n.net.batchnorm_train_layers() == ["prefinal-chain", "prefinal-xent"]
    n.net.set_batchnorm_train(True)
    n.forward()
    acts, relu, stats = n.acts(), n.net.relu_masks(), n.governed_stats()
    xg = (np.random.default_rng(8).standard_normal((T, 200)) * 0.05).astype(np.float16)
    xb = kf.upload_fp16(xg)
    n.net.backward(n.gb.ptr, xb.ptr)
    grads = n.net.read_grads()
    tp = {k: synth.trunc_fp16(v).astype(np.float64) for k, v in n.params.items()}
    x = acts["prefinal-l"].astype(np.float64)
    gin = 0.0
    for pre, out, seed in (("prefinal-xent", "output-xent", xg), ("prefinal-chain", "output", n.og)):
        f = bs.prefinal_forward(x, tp[pre + ".BigW"], tp[pre + ".BigBias"].reshape(-1), tp[pre + ".SmallW"])
        assert rel_fro(acts[pre], f["act"]) <= 2e-3 and max_abs_rel(acts[pre], f["act"]) <= 1e-2, pre
        for which in (0, 1):
            em, ev = _stat_errors((pre, which), stats[(pre, which)], f["stats%d" % which])
            assert em <= 2e-3 and ev <= 2e-3, (pre, which, em, ev)
        f = bs.prefinal_forward(x, tp[pre + ".BigW"], tp[pre + ".BigBias"].reshape(-1), tp[pre + ".SmallW"], force_mask=relu[pre])
        g = seed.astype(np.float64)
        want = {out + ".W": f["act"].T @ g, out + ".Bias": g.sum(0).reshape(1, -1)}
        gW, gb, gW2, gi = bs.prefinal_backward(bs.f16(g @ tp[out + ".W"].T), f)
        want.update({pre + ".BigW": gW, pre + ".BigBias": gb.reshape(1, -1), pre + ".SmallW": gW2})
        gin = gin + gi
        for k, v in want.items():
            e = rel_fro(grads[k], v)
            print("%s: %.2e" % (k, e))
            assert e <= 5e-3, (k, e)
    e = rel_fro(grads["prefinal-l.W"], acts["tdnnf4"].astype(np.float64).T @ bs.f16(gin))
    print("prefinal-l.W: %.2e" % e)
    assert e <= 5e-3
    n.close()


# ---------------------------------------------------------------------------
# the default sites, mode hygiene
# ---------------------------------------------------------------------------
def test_default_sites_are_the_tdnnf_layers_bit_for_bit(gpu):
    kf = gpu
    a, b = Net(kf, "tiny.xconfig"), Net(kf, "tiny.xconfig")
    tdnnf = ["tdnnf5", "tdnnf6", "tdnnf7", "tdnnf8"]
    assert a.net.batchnorm_train_layers() == tdnnf and a.net.batchnorm_train_sites() == 1
    a.net.set_batchnorm_train(True)          # a never sees the new calls
    b.net.set_batchnorm_train_sites("all")
    b.net.set_batchnorm_train_sites("tdnnf")
    assert b.net.batchnorm_train_layers() == tdnnf
    b.net.set_batchnorm_train(True)
    (aa, ga), (ab, gb) = a.run(), b.run()
    for k in aa:
        assert _same(aa[k], ab[k]), k
    for k in ga:
        assert _same(ga[k], gb[k]), k
    with pytest.raises(kf.KfError, match="does not govern"):
        b.net.batchnorm_batch_stats("cnn1")
    a.close(), b.close()


@pytest.mark.parametrize("cfg", ["tiny.xconfig", "tiny_ivec.xconfig"])
def test_mode_hygiene(gpu, cfg):
    """off after on equals never on, bit for bit: activations, gradients and the frozen scale /
    shift of every governed BatchNorm; two train-mode steps agree bit for bit, with the weight
    gradients on their own stream or not"""
    kf = gpu
    n = Net(kf, cfg)
    net = n.net

    def frozen_pairs():
        out = {}
        for i, (name, *_r) in enumerate(net.layers):
            for what in ("bn_scale", "bn_shift", "bn2_scale", "bn2_shift"):
                p = kf.nnet.nnet_debug_tensor(net.h, what.encode(), i)
                if p:
                    d = kf.nnet.nnet_bn_dim(net.h, name.encode(), 1 if "2" in what else 0)
                    out[(name, what)] = kf.read_f32(p, (d,))
        return out

    a0, g0 = n.run()
    p0 = frozen_pairs()
    assert ("cnn1", "bn_shift") in p0 and ("prefinal-chain", "bn2_scale") in p0 and ("idct-batchnorm", "bn_scale") in p0
    net.set_batchnorm_train_sites("all")
    net.set_batchnorm_train(True)
    with pytest.raises(kf.KfError, match="switch it off first"):
        net.set_batchnorm_train_sites("conv")
    a1, g1 = n.run()
    # (the frozen statistics are init_network's random ones: the train-mode forward is far from the
    # frozen one, not two roundings of it)
    for name in ("idct-batchnorm", "cnn1", "cnn2", "prefinal-chain", "output"):
        assert rel_fro(a1[name], a0[name]) >= 5e-2, (name, rel_fro(a1[name], a0[name]))
    a2, g2 = n.run()
    net.set_wgrad_stream(False)
    a3, g3 = n.run()
    net.set_wgrad_stream(True)
    for a, g in ((a2, g2), (a3, g3)):
        for k in a1:
            assert _same(a[k], a1[k]), k
        for k in g1:
            assert _same(g[k], g1[k]), k
    net.set_batchnorm_train(False)
    a4, g4 = n.run()
    for k in a0:
        assert _same(a4[k], a0[k]), k
    for k in g0:
        assert _same(g4[k], g0[k]), k
    p4 = frozen_pairs()
    assert all(_same(p4[k], p0[k]) for k in p0)
    net.set_batchnorm_train_sites("conv")      # allowed again; the list follows
    assert all(name.startswith("cnn") for name in net.batchnorm_train_layers())
    n.close()


# ---------------------------------------------------------------------------
# accumulators and commit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["tiny.xconfig", "tiny_ivec.xconfig"])
def test_accumulators_and_commit(gpu, cfg):
    kf = gpu
    n = Net(kf, cfg)
    net = n.net
    net.set_batchnorm_train_sites("all")
    net.set_batchnorm_train(True)
    net.batchnorm_zero_stats()
    gov = net.batchnorm_train_layers()
    bns = [(name, w) for name in gov for w in ((0, 1) if name.startswith("prefinal") else (0,))]
    hout = {"cnn1": 40, "cnn2": 20, "cnn3": 20, "cnn4": 10}
    second = Net(kf, cfg, frames=210, seq=np.asarray([0, 100, 210], np.int32))   # (only its inputs are used)
    want = {k: [0.0, 0.0] for k in bns}
    for src, frames, B in ((n, 300, 3), (second, 210, 2)):
        if src.ib is not None:
            net.forward_ivector(src.fb.ptr, frames, src.ib.ptr, src.seq)
        else:
            net.forward(src.fb.ptr, frames)
        for name, w in bns:
            cnt = B if name == "ivector-batchnorm" else frames * hout.get(name, 1)
            m, v = (s.astype(np.float64) for s in net.batchnorm_batch_stats(name, w))
            want[(name, w)][0] = want[(name, w)][0] + cnt * m
            want[(name, w)][1] = want[(name, w)][1] + cnt * (v + m * m)
    second.close()
    pooled = {}
    for name, w in bns:
        cnt, s, q = net.batchnorm_stats(name, w)
        assert cnt == (5 if name == "ivector-batchnorm" else 510 * hout.get(name, 1)), (name, cnt)
        assert s.size == kf.nnet.nnet_bn_dim(net.h, name.encode(), w)
        assert np.linalg.norm(s - want[(name, w)][0]) <= 1e-6 * np.linalg.norm(want[(name, w)][0]), name
        assert np.linalg.norm(q - want[(name, w)][1]) <= 1e-6 * np.linalg.norm(want[(name, w)][1]), name
        mu = s / cnt
        pooled[(name, w)] = (mu.astype(np.float32), np.maximum(q / cnt - mu * mu, 0.0).astype(np.float32))
    assert net.batchnorm_commit() == len(gov)
    net.set_batchnorm_train(False)
    n.forward()
    got = n.acts()
    # the frozen forward of a fresh network fed the same statistics through set_bn
    f = Net(kf, cfg)
    for (name, w), (m, v) in pooled.items():
        f.net.set_bn(name, w, m, v, np.ones_like(m), np.zeros_like(m), eps=1e-3)
    f.forward()
    want_acts = f.acts()
    f.close()
    for k in want_acts:
        assert _same(got[k], want_acts[k]), k
    # the frozen forward does not accumulate; zero_stats clears; nothing left to commit
    assert net.batchnorm_stats("cnn1")[0] == 510 * 40
    net.batchnorm_zero_stats()
    for name, w in bns:
        cnt, s, q = net.batchnorm_stats(name, w)
        assert cnt == 0 and not s.any() and not q.any()
    assert net.batchnorm_commit() == 0
    n.close()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    """the frame-level batchnorm-component above a trainable layer; MXFP8, implicit dz, row
    subsampling and nnet_backward_n with every site governed, in either order"""
    kf = gpu
    from kfp16 import synth
    base = synth.load_xconfig("tiny.xconfig")
    # (tdnnf8 at time-stride 3, so that the net admits row subsampling at all)
    xcfg = base.replace("name=tdnnf8 dim=256 bottleneck-dim=64 time-stride=1", "name=tdnnf8 dim=256 bottleneck-dim=64 time-stride=3")
    assert xcfg != base
    n = Net(kf, None, xcfg=xcfg)
    net, fb, gb = n.net, n.fb, n.gb
    net.set_batchnorm_train_sites("all")
    net.set_batchnorm_train(True)
    net.forward(fb.ptr, T)
    for call in (lambda: net.set_fp8(True), lambda: net.set_implicit_dz(True), lambda: net.set_row_subsampling(3),
                 lambda: kf.check(kf.nnet.nnet_backward_n(net.h, gb.ptr, 2), "nnet_backward_n")):
        with pytest.raises(kf.KfError, match="nnet_set_bn_train"):
            call()
    net.backward(gb.ptr)                  # the net still works
    net.set_batchnorm_train(False)
    for on, off, name in ((lambda: net.set_fp8(True), lambda: net.set_fp8(False), "nnet_set_fp8"),
                          (lambda: net.set_implicit_dz(True), lambda: net.set_implicit_dz(False), "nnet_set_implicit_dz"),
                          (lambda: net.set_row_subsampling(3), lambda: net.set_row_subsampling(0), "nnet_set_row_subsampling")):
        on()
        with pytest.raises(kf.KfError, match=name):
            net.set_batchnorm_train(True)
        off()
    net.set_batchnorm_train(True)
    n.run()
    kf.sync()
    n.close()
    # the switch set while it governs nothing stays a switch: the sites may still change, and the
    # mode then goes on for them
    z = Net(kf, "tiny.xconfig")
    z.net.set_batchnorm_train_sites(0)
    assert z.net.batchnorm_train_layers() == []
    z.net.set_batchnorm_train(True)
    z.net.set_batchnorm_train_sites("conv")
    assert z.net.batchnorm_train_layers() == ["cnn1", "cnn2", "cnn3", "cnn4"]
    z.run()
    assert z.net.batchnorm_stats("cnn2")[0] == T * 20
    with pytest.raises(kf.KfError, match="switch it off first"):
        z.net.set_batchnorm_train_sites("all")
    z.close()
    # a batchnorm-component between a linear-component and the prefinal layer
    mid = base.replace("prefinal-layer name=prefinal-chain input=prefinal-l",
                       "batchnorm-component name=mid-bn input=prefinal-l\nprefinal-layer name=prefinal-chain input=mid-bn")
    assert mid != base
    m = Net(kf, None, xcfg=mid)
    m.net.set_batchnorm_train_sites("all")
    with pytest.raises(kf.KfError, match="mid-bn"):
        m.net.set_batchnorm_train(True)
    m.run()                               # still frozen, and working
    m.net.set_batchnorm_train_sites(["tdnnf", "conv", "prefinal"])
    m.net.set_batchnorm_train(True)
    m.run()
    kf.sync()
    m.close()


def test_refusal_data_parallel(gpu):
    kf = gpu
    from kfp16 import dp
    n = Net(kf, "tiny.xconfig")
    n.net.set_batchnorm_train_sites("all")
    comm = dp.Communicator(0, 1, dp.unique_id(), 0)
    n.net.bind_dp(comm, 1 << 20)
    with pytest.raises(kf.KfError, match="nnet_bind_dp"):
        n.net.set_batchnorm_train(True)
    n.net.bind_dp(None, 0)
    n.net.set_batchnorm_train(True)
    with pytest.raises(kf.KfError, match="nnet_set_bn_train"):
        n.net.bind_dp(comm, 1 << 20)
    comm.close()
    n.close()


# ---------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------
def test_trainer_composition(gpu, tmp_path):
    """EgsTrainer, three steps with every site in training mode, the Kaldi update, natural gradient,
    the orthonormal constraint at every step, a dropout schedule and xent_regularize together"""
    kf = gpu
    import egs_writer as W
    from kfp16 import egs, synth, trainer
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, 4, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=4).next_batch()
    den = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)
    assert trainer.TrainConfig().batchnorm_train_sites == "tdnnf"
    cfg = trainer.TrainConfig(learning_rate=1e-3, momentum=0.9, kaldi_update=True, max_param_change=1.0,
                              natural_gradient=True, orthonormal_every=1, dropout_schedule="0,0.3", dropout_seed=11,
                              total_steps=4, batchnorm_train=True, batchnorm_train_sites="all", xent_regularize=0.1)
    xcfg = synth.load_xconfig("tiny_xent.xconfig")
    assert xcfg.count("bypass-scale=0.66") == 2
    xcfg = xcfg.replace("bypass-scale=0.66", "bypass-scale=0.66 dropout-proportion=0.0")
    tr = trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=800, config=cfg)
    synth.init_network(tr.net)
    gov = tr.net.batchnorm_train_layers()
    assert gov == ["idct-batchnorm", "cnn1", "cnn2", "tdnnf3", "tdnnf4", "prefinal-chain", "prefinal-xent"]
    for step in range(3):
        tr.step(batch, fraction=(step + 1) / 4)
        r = tr.result()
        assert r.num_ok == batch.batch_size and np.isfinite(r.objf) and np.isfinite(r.xent_objf)
        stats = tr.net.natural_gradient_stats()
        assert stats and not any(s["flag"] for s in stats)
        assert tr.net.batchnorm_stats("cnn2")[0] == (step + 1) * batch.total_frames * 20
        assert tr.net.batchnorm_stats("prefinal-xent", 1)[0] == (step + 1) * batch.total_frames
    assert tr.commit_batchnorm() == len(gov)
