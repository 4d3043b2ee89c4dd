"""EgsTrainer with TrainConfig.loss_scale on configs/tiny.xconfig and
tiny_xent.xconfig: four egs of the writer fixture (rows 150, 183, 129, P = 200).

  * loss_scale = 0 is the trainer as it was, bit for bit.
  * a fixed scale of 256: the objective is unchanged and the parameter change of one step agrees
    with the scaling-off trainer's at the weight-gradient bar of DESIGN §3, rel-Frobenius 5e-3 per
    tensor, with sgd and with the Kaldi update, with xent_regularize, row subsampling and
    training-mode BatchNorm.
  * a scale of 2^20 overflows: the step is skipped bit for bit, the scale halves until a step
    succeeds (at most 21 halvings lead from 2^20 to 1).
  * supervision_weight = 2^-12 (the underflow the feature is for): the gradient buffer at scale
    2^12, divided by it, meets 5e-3 against the weight-1 buffer times 2^-12; without the scale
    the error is larger.
  * natural gradient and MXFP8 mode are refused in both orders.
"""
import numpy as np
import pytest

from conftest import rel_fro

pytestmark = pytest.mark.gpu

BAR = 5e-3     # weight gradients, relative Frobenius per tensor
HUGE = 1 << 30


@pytest.fixture(scope="module")
def egs(tmp_path_factory):
    import egs_writer as W
    from kfp16 import egs, synth
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, 4, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    d = tmp_path_factory.mktemp("ls")
    W.write_ark(d / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(d / "cegs.*.ark"), batch_size=4).next_batch()
    return batch, synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)


def _trainer(egs, xcfg="tiny.xconfig", **kw):
    from kfp16 import synth, trainer
    kw.setdefault("learning_rate", 1e-2)
    kw.setdefault("momentum", 0.9)
    tr = trainer.EgsTrainer(synth.load_xconfig(xcfg), egs[1], max_egs=8, max_frames=800,
                            config=trainer.TrainConfig(**kw))
    synth.init_network(tr.net)
    return tr


def _state(gpu, tr):
    """master, fp16 weights and velocity, as bits"""
    from kfp16 import nnet
    gpu.sync()
    n = tr.net.num_params
    return dict(w32=gpu.read_f32(tr.net.master_ptr, (n,)).view(np.uint32),
                w16=gpu.read_fp16(nnet.nnet_weight_buffer(tr.net.h), (n,)).view(np.uint16),
                v=gpu.read_f32(nnet.nnet_debug_tensor(tr.net.h, b"vel", 0), (n,)).view(np.uint32))


def _same_state(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def test_off_is_off(gpu, egs):
    """loss_scale = 0 for 3 steps: the parameters, fp16 weights and velocity of a trainer built
    without the field"""
    from kfp16 import KfError
    outs = []
    for kw in ({}, dict(loss_scale=0.0, loss_scale_growth_interval=7)):
        tr = _trainer(egs, **kw)
        for _ in range(3):
            tr.step(egs[0])
        outs.append((_state(gpu, tr), tr.result().objf))
        assert tr.net.loss_scale_ptr() is None
        with pytest.raises(KfError, match="loss scale is off"):
            tr.loss_scale_stats()
        tr.net.close()
    _same_state(outs[0][0], outs[1][0], "loss_scale=0")
    assert outs[0][1] == outs[1][1]


VARIANTS = {
    "plain": ("tiny.xconfig", {}),
    "xent": ("tiny_xent.xconfig", dict(xent_regularize=0.1)),
    # (tiny.xconfig's tdnnf8 has time-stride 1, which the row set does not cover; without
    # xent_regularize the xent branch of tiny_xent.xconfig gets no gradient)
    "rsub": ("tiny_xent.xconfig", dict(row_subsampling=True, xent_regularize=0.1)),
    "bn": ("tiny.xconfig", dict(batchnorm_train=True)),
}


@pytest.mark.parametrize("kaldi_update", [False, True], ids=["sgd", "update"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_scaled_step_matches_the_unscaled_one(gpu, egs, variant, kaldi_update):
    xcfg, kw = VARIANTS[variant]
    kw = dict(kw, kaldi_update=kaldi_update, max_param_change=2.0 if kaldi_update else 0.0)
    res = []
    for ls in (0.0, 256.0):
        tr = _trainer(egs, xcfg, loss_scale=ls, loss_scale_growth_interval=HUGE if ls else 2000, **kw)
        p0 = tr.net.get_params()
        tr.step(egs[0])
        r = tr.result()
        p1 = tr.net.get_params()
        stats = tr.loss_scale_stats() if ls else None
        res.append((r, {k: p1[k].astype(np.float64) - p0[k] for k in p0}, stats))
        tr.net.close()
    (r0, d0, _), (r1, d1, st) = res
    assert st == dict(scale=256.0, since=1, steps=1, skipped=0, last_overflow=False)
    assert r0.num_ok == egs[0].batch_size and np.isfinite(r0.objf)
    assert (r1.objf, r1.total_weight, r1.num_logprob, r1.den_logprob) == \
        (r0.objf, r0.total_weight, r0.num_logprob, r0.den_logprob)
    if variant == "xent":
        assert (r1.xent_objf, r1.xent_weight) == (r0.xent_objf, r0.xent_weight)
    worst = ("", 0.0)
    for k, d in d0.items():
        assert np.any(d), f"{k}: the unscaled step did not move it"
        e = rel_fro(d1[k], d)
        worst = max(worst, (k, e), key=lambda t: t[1])
    print(f"{variant} {'update' if kaldi_update else 'sgd'}: largest rel-Frobenius of the change {worst[1]:.2e} ({worst[0]})")
    for k, d in d0.items():
        assert rel_fro(d1[k], d) <= BAR, (k, rel_fro(d1[k], d))


def test_overflow_skips_until_the_scale_fits(gpu, egs):
    tr = _trainer(egs, kaldi_update=True, max_param_change=2.0, loss_scale=256.0, loss_scale_growth_interval=HUGE)
    tr.step(egs[0])                                      # a clean step: the velocity is not zero
    before = _state(gpu, tr)
    assert np.any(before["v"]) and tr.loss_scale_stats()["skipped"] == 0
    ptr = tr.net.loss_scale_ptr()
    tr.net.set_loss_scale(True, init_scale=256.0, growth_interval=HUGE, max_scale=float(2 ** 20))
    assert tr.net.loss_scale_ptr() == ptr                # the state is allocated once
    tr.net.set_loss_scale_value(65536.0 * 2 ** 4)
    assert tr.loss_scale_stats()["scale"] == 2.0 ** 20
    tr.step(egs[0])
    r = tr.result()
    assert np.isfinite(r.objf) and r.num_ok == egs[0].batch_size    # the objective itself is not scaled
    _same_state(_state(gpu, tr), before, "skipped step")
    st = tr.loss_scale_stats()
    assert st == dict(scale=2.0 ** 19, since=0, steps=1, skipped=1, last_overflow=True)
    us = tr.net.update_stats()
    assert not np.any(us["norms"]) and not np.any(us["scales"]) and us["global_norm"] == 0 and us["global_scale"] == 0
    assert tr.steps == 2                                 # a skipped step counts
    for _ in range(21):                                  # 20 more skipped steps at the most, then a clean one
        if not st["last_overflow"]:
            break
        tr.step(egs[0])
        st = tr.loss_scale_stats()
    print(f"overflow: {st['skipped']} skipped steps, the first clean one at scale {st['scale']:g}")
    assert not st["last_overflow"], "no step succeeded after 21 skipped ones"
    assert st["skipped"] <= 21 and st["steps"] == st["skipped"] + 1 and st["since"] == 1
    assert st["scale"] == 2.0 ** (20 - st["skipped"]) and tr.steps == 1 + st["steps"]
    after = _state(gpu, tr)
    assert np.any(after["w32"] != before["w32"])
    assert all(np.all(np.isfinite(v)) for v in tr.net.get_params().values())
    assert np.all(np.isfinite(after["v"].view(np.float32)))
    tr.net.close()


def _grads(gpu, egs, weight, ls):
    """the gradient buffer of one step (learning rate 0) at supervision weight `weight`"""
    from kfp16 import chain
    opts = chain.KfChainOpts(0.0, 0.0, 1e-5, 0.0, weight)    # (the out-of-range penalty is not scaled by the weight)
    tr = _trainer(egs, learning_rate=0.0, momentum=0.0, opts=opts, loss_scale=ls, loss_scale_growth_interval=HUGE if ls else 2000)
    tr.step(egs[0])
    gpu.sync()
    g = tr.net.read_grads()
    if ls:
        assert tr.loss_scale_stats()["skipped"] == 0
    tr.net.close()
    return {k: v.astype(np.float64) for k, v in g.items()}


def test_underflow_is_what_the_scale_repairs(gpu, egs):
    """supervision_weight 2^-12: reference = the scaling-off buffer at weight 1 times 2^-12 (the
    existing path, held to the oracle by the existing tests)"""
    w = 2.0 ** -12
    ref = {k: v * w for k, v in _grads(gpu, egs, 1.0, 0.0).items()}
    on = {k: v / 2.0 ** 12 for k, v in _grads(gpu, egs, w, 2.0 ** 12).items()}
    off = _grads(gpu, egs, w, 0.0)
    e_on = {k: rel_fro(on[k], ref[k]) for k in ref}
    e_off = {k: rel_fro(off[k], ref[k]) for k in ref}
    for k in ref:
        print(f"{k:24s} rel-Frobenius unscaled {e_off[k]:.3e}   scale 2^12 {e_on[k]:.3e}")
    assert all(np.any(v) for v in ref.values())
    assert max(e_off.values()) > BAR, "at this weight the unscaled step loses nothing: lower it"
    for k in ref:
        assert e_on[k] <= BAR, (k, e_on[k])
    assert sum(e_off.values()) > sum(e_on.values())


def test_refusals_in_both_orders(gpu):
    from kfp16 import KfError, Network, synth
    xcfg = synth.load_xconfig("tiny.xconfig")
    for other, on, off, phrase in (("natural gradient", lambda n: n.set_natural_gradient(True),
                                    lambda n: n.set_natural_gradient(False), "natural gradient"),
                                   ("fp8", lambda n: n.set_fp8(True), lambda n: n.set_fp8(False), "MXFP8")):
        net = Network(xcfg, max_frames=120)
        synth.init_network(net)
        on(net)
        with pytest.raises(KfError, match=f"set_loss_scale: not supported .*{phrase}"):
            net.set_loss_scale(True)
        assert net.loss_scale_ptr() is None
        off(net)
        net.set_loss_scale(True)
        assert net.loss_scale_ptr() and net.loss_scale_stats()["scale"] == 65536.0
        with pytest.raises(KfError, match="not supported with the loss scale on"):
            on(net)
        net.set_loss_scale(False)
        on(net)                                          # turning the loss scale off lifts the refusal
        net.close()


def test_trainer_refuses_natural_gradient(gpu, egs):
    from kfp16 import trainer
    with pytest.raises(ValueError, match="natural_gradient"):
        trainer.TrainConfig(loss_scale=256.0, natural_gradient=True)
