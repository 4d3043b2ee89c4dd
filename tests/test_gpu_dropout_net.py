"""Per-sequence dropout of the TDNN-F layers at network level (kf_nnet.h nnet_set_dropout,
DESIGN.md §21): tiny.xconfig with dropout-proportion on its four tdnnf-layers, three sequences
of unequal length, p = 0.3. The reference (tests/dropout_ref.py DropoutOracle) runs the
committed CPU oracle layer by layer with the masks read back from the net; tolerances are
test_gpu_nnet.py's for the same tensors (activations 2e-3 relative Frobenius and 1e-2 of the
largest value, gradients 5e-3)."""
import numpy as np
import pytest

import dropout_ref as dr
from conftest import max_abs_rel, rel_fro

pytestmark = pytest.mark.gpu

TDNNF = ["tdnnf5", "tdnnf6", "tdnnf7", "tdnnf8"]
SEQ = [0, 40, 97, 150]
SEED, P = 0x5EED5EED12345678, 0.3


def _xcfg(extra=""):
    from kfp16 import synth
    x = synth.load_xconfig("tiny.xconfig")
    assert x.count("bypass-scale=0.66") == 4
    return x.replace("bypass-scale=0.66", "bypass-scale=0.66 dropout-proportion=0.0" + extra)


def _net(kfp16, xcfg, T, seq=SEQ, p=P, on=True, seed=SEED):
    from kfp16 import synth
    net = kfp16.Network(xcfg, max_frames=T)
    params, bns = synth.init_network(net)
    if seq is not None:
        net.set_sequences(seq)
    if net.dropout_layers():
        net.set_dropout_proportion(p)
    net.set_dropout(on, seed)
    return net, params, bns


def _out_grad(kfp16, T, Pdim, seed=7, rows=None):
    og = (np.random.default_rng(seed).standard_normal((T, Pdim)) * 0.05).astype(np.float16)
    if rows is not None:   # supervised rows only
        z = np.zeros_like(og)
        z[rows] = og[rows]
        og = z
    return og


def test_forward_backward_against_reference(gpu):
    kfp16 = gpu
    import oracle  # noqa: F401  (DropoutOracle imports it)
    from kfp16 import synth
    T = SEQ[-1]
    xcfg = _xcfg()
    net, params, bns = _net(kfp16, xcfg, T)
    assert net.dropout_layers() == TDNNF
    feats = synth.make_features(T, 40)
    fb = kfp16.upload_fp16(feats)
    net.forward(fb.ptr, T)
    assert net.dropout_step() == 1
    masks = {n: net.dropout_mask(n) for n in TDNNF}
    for i, n in enumerate(TDNNF):   # the masks are the rule's, for (seed, step 0, the layer's ordinal)
        ref = dr.dropout_masks(SEED, 0, i, len(SEQ) - 1, 256, P)
        assert masks[n].shape == ref.shape
        assert np.all(np.abs(masks[n] - ref) <= np.spacing(np.maximum(np.abs(ref), np.abs(masks[n])))), n
    tp = {k: synth.trunc_fp16(v) for k, v in params.items()}
    on = dr.DropoutOracle(xcfg, tp, bns, masks, SEQ, threads=16)
    on.forward(feats.astype(np.float32))
    relu = net.relu_masks()
    for name in TDNNF + ["prefinal-l", "prefinal-chain", "output"]:
        got, ref = net.read_activation(name).astype(np.float32), on.act(name)
        print("%s: rel fro %.2e, max abs rel %.2e" % (name, rel_fro(got, ref), max_abs_rel(got, ref)))
        assert rel_fro(got, ref) <= 2e-3, (name, rel_fro(got, ref))
        assert max_abs_rel(got, ref) <= 1e-2, (name, max_abs_rel(got, ref))
    # the masks did something: without them the activations are far from the reference
    plain, _, _ = _net(kfp16, xcfg, T, on=False)
    plain.forward(fb.ptr, T)
    assert rel_fro(plain.read_activation("tdnnf8").astype(np.float32), on.act("tdnnf8")) > 0.05
    plain.close()
    on.close()
    # backward with the product's ReLU decisions replayed, as test_gpu_nnet.py does
    on = dr.DropoutOracle(xcfg, tp, bns, masks, SEQ, threads=16)
    on.forward(feats.astype(np.float32), force_masks=relu)
    og = _out_grad(kfp16, T, 200)
    gb = kfp16.upload_fp16(og)
    net.backward(gb.ptr)
    got = net.read_grads()
    ref = on.backward(og.astype(np.float32))
    errs = {k: rel_fro(got[k], ref[k]) for k in ref}
    print("grad errors: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    # every trainable tensor, the conv stack's among them: they see the gradient into cnn4
    assert set(errs) == set(got)
    bad = {k: v for k, v in errs.items() if v > 5e-3}
    assert not bad, bad
    on.close()
    net.close()


def test_mask_shared_by_the_frames_of_a_sequence(gpu):
    """tdnnf5 has no bypass and its input does not depend on dropout: its activation with
    dropout is the one without times mask[sequence of the row], to an fp16 rounding each"""
    kfp16 = gpu
    from kfp16 import synth
    T = SEQ[-1]
    xcfg = _xcfg()
    fb = kfp16.upload_fp16(synth.make_features(T, 40))
    net, _, _ = _net(kfp16, xcfg, T)
    net.forward(fb.ptr, T)
    y1 = net.read_activation("tdnnf5").astype(np.float64)
    m = net.dropout_mask("tdnnf5")
    assert m.shape == (3, 256) and m.min() >= 1 - 2 * P - 1e-6 and m.max() <= 1 + 2 * P + 1e-6
    assert not np.array_equal(m[0], m[1]) and not np.array_equal(m[1], m[2])
    net.set_dropout(False)
    net.forward(fb.ptr, T)
    y0 = net.read_activation("tdnnf5").astype(np.float64)
    seg = dr.row_segments(SEQ, T)
    want = y0 * m[seg]
    # y0 and y1 each carry one fp16 rounding of the same fp32 value (times the mask)
    tol = (np.abs(y0) * 2.0 ** -11 + 2.0 ** -24) * m[seg] + np.abs(want) * 2.0 ** -11 + 2.0 ** -24
    assert np.all(np.abs(y1 - want) <= tol * 1.01)
    # and the wrong sequence's mask does not fit
    wrong = y0 * m[(seg + 1) % 3]
    assert np.mean(np.abs(y1 - wrong) > tol * 1.01) > 0.5
    net.close()


def test_off_paths_bit_identical_and_replay(gpu):
    """dropout off after on, and p = 0 while on, give the outputs and gradients of a net that
    never had a component, bit for bit; (seed, step) replays a forward / backward exactly, with
    the weight gradients on their own stream or not"""
    kfp16 = gpu
    from kfp16 import synth
    T = SEQ[-1]
    fb = kfp16.upload_fp16(synth.make_features(T, 40))
    gb = kfp16.upload_fp16(_out_grad(kfp16, T, 200))

    def run(net):
        net.forward(fb.ptr, T)
        out = net.read_activation("output").copy()
        net.backward(gb.ptr)
        return out, net.read_grads()

    never, _, _ = _net(kfp16, synth.load_xconfig("tiny.xconfig"), T, on=False)
    o0, g0 = run(never)
    never.close()
    net, _, _ = _net(kfp16, _xcfg(), T)
    o1, g1 = run(net)                     # step 0, p = 0.3
    assert not np.array_equal(o1, o0)
    net.set_dropout(False, SEED)
    o2, g2 = run(net)                     # off: the step does not advance
    assert net.dropout_step() == 1
    net.set_dropout(True, SEED)
    net.set_dropout_proportion(0.0)
    o3, g3 = run(net)                     # on with p = 0: the step advances, nothing is drawn
    assert net.dropout_step() == 2
    with pytest.raises(kfp16.KfError, match="no mask"):
        net.dropout_mask("tdnnf6")
    for o, g in ((o2, g2), (o3, g3)):
        assert np.array_equal(o.view(np.uint16), o0.view(np.uint16))
        for k in g0:
            assert np.array_equal(g[k], g0[k]), k
    # replay of step 0; another step and another seed differ
    net.set_dropout_proportion(P)
    net.set_dropout_step(0)
    net.set_wgrad_stream(False)
    o4, g4 = run(net)
    net.set_wgrad_stream(True)
    assert np.array_equal(o4, o1) and all(np.array_equal(g4[k], g1[k]) for k in g1)
    o5, _ = run(net)                      # step 1
    assert not np.array_equal(o5, o1)
    net.set_dropout(True, SEED + 1)
    net.set_dropout_step(0)
    o6, _ = run(net)
    assert not np.array_equal(o6, o1)
    # a forward whose T is not the boundaries' fails while dropout is on
    with pytest.raises(kfp16.KfError, match="nnet_set_sequences"):
        net.forward(fb.ptr, T - 1)
    net.set_sequences(None)               # one sequence: a single mask row
    net.forward(fb.ptr, T - 1)
    assert net.dropout_mask("tdnnf7").shape == (1, 256)
    net.close()


def test_row_subsampling_matches_full_rows(gpu):
    """the TDNN-F stack on the compact row set (tdnnf8 at time-stride 3, so that it is part of
    it): rows of the set and every weight gradient as on full rows with the same (seed, step), to
    test_gpu_row_subsampling.py's bounds (rows bit-identical, gradients 1e-5)"""
    kfp16 = gpu
    from kfp16 import synth
    T = 300                                # (T - 1) % 3 == 2: with a tail
    seq = [0, 61, 190, T]
    xcfg = _xcfg().replace("name=tdnnf8 dim=256 bottleneck-dim=64 time-stride=1", "name=tdnnf8 dim=256 bottleneck-dim=64 time-stride=3")
    assert "time-stride=1" not in xcfg
    fb = kfp16.upload_fp16(synth.make_features(T, 40))
    sup = np.arange(30, T, 3)
    og = _out_grad(kfp16, T, 200, rows=sup)
    res = {}
    for sub in (False, True):
        net, _, _ = _net(kfp16, xcfg, T, seq=seq)
        if sub:
            net.set_row_subsampling(3)
        net.forward(fb.ptr, T)
        tc, tc0, rows = net.row_set()
        assert (tc > 0) == sub, "the row set was not used: T too small for its guard"
        acts = {n: net.read_activation(n) for n in TDNNF + ["output"]}
        gb = kfp16.upload_fp16(og[rows] if sub else og)
        net.backward(gb.ptr)
        kfp16.sync()
        res[sub] = dict(acts=acts, grads=net.read_grads(), rows=rows, tc0=tc0, masks=[net.dropout_mask(n) for n in TDNNF])
        net.close()
    full, cs = res[False], res[True]
    rows, tc0 = cs["rows"], cs["tc0"]
    for a, b in zip(full["masks"], cs["masks"]):
        assert np.array_equal(a, b)
    for n in TDNNF + ["output"]:
        assert cs["acts"][n].shape[0] == len(rows), n     # the layer ran on the compact rows
        assert np.array_equal(cs["acts"][n][:tc0].view(np.uint16), full["acts"][n][rows[:tc0]].view(np.uint16)), n
    for k, v in full["grads"].items():
        assert rel_fro(cs["grads"][k], v) <= 1e-5, (k, rel_fro(cs["grads"][k], v))


def test_conflicts(gpu):
    """MXFP8, implicit dz and nnet_backward_n with dropout: an error in either order"""
    kfp16 = gpu
    from kfp16 import synth
    T = SEQ[-1]
    net, _, _ = _net(kfp16, _xcfg(), T)
    fb = kfp16.upload_fp16(synth.make_features(T, 40))
    gb = kfp16.upload_fp16(_out_grad(kfp16, T, 200))
    net.forward(fb.ptr, T)
    with pytest.raises(kfp16.KfError, match="dropout"):
        net.set_fp8(True)
    with pytest.raises(kfp16.KfError, match="dropout"):
        net.set_implicit_dz(True)
    with pytest.raises(kfp16.KfError, match="dropout"):
        kfp16.check(kfp16.nnet.nnet_backward_n(net.h, gb.ptr, 2), "nnet_backward_n")
    net.backward(gb.ptr)                  # the net still works
    net.set_dropout(False)
    kfp16.check(kfp16.nnet.nnet_backward_n(net.h, gb.ptr, 2), "nnet_backward_n")
    net.set_implicit_dz(True)
    with pytest.raises(kfp16.KfError, match="implicit dz"):
        net.set_dropout(True, 1)
    net.set_implicit_dz(False)
    net.set_fp8(True)
    with pytest.raises(kfp16.KfError, match="MXFP8"):
        net.set_dropout(True, 1)
    net.set_fp8(False)
    net.set_dropout(True, 1)
    net.forward(fb.ptr, T)
    net.backward(gb.ptr)
    kfp16.sync()
    net.close()
    # a net without a component takes every mode with the switch on
    plain, _, _ = _net(kfp16, synth.load_xconfig("tiny.xconfig"), T, on=True)
    plain.set_implicit_dz(True)
    plain.forward(fb.ptr, T)
    kfp16.check(kfp16.nnet.nnet_backward_n(plain.h, gb.ptr, 2), "nnet_backward_n")
    kfp16.sync()
    plain.close()


def test_natural_gradient_with_dropout(gpu):
    kfp16 = gpu
    from kfp16 import synth
    T = SEQ[-1]
    net, _, _ = _net(kfp16, _xcfg(), T)
    net.set_natural_gradient(True)
    fb = kfp16.upload_fp16(synth.make_features(T, 40))
    gb = kfp16.upload_fp16(_out_grad(kfp16, T, 200))
    net.forward(fb.ptr, T)
    net.backward(gb.ptr)
    stats = net.natural_gradient_stats()
    assert stats and not any(s["flag"] for s in stats)
    g = net.read_grads()
    assert all(np.isfinite(v).all() for v in g.values()) and any(np.abs(v).max() > 0 for v in g.values())
    net.close()


def test_trainer_schedule(gpu, tmp_path):
    """EgsTrainer with a dropout schedule on the egs fixture of test_gpu_egs_train.py: the
    proportion reaches the net, one mask row per eg, a finite objective, new masks each step"""
    kf = gpu
    import egs_writer as W
    from kfp16 import egs, synth, trainer
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, 6, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=6).next_batch()
    den = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)
    # (learning rate 0: the fixture's fixed batch diverges within three plain SGD steps at 1e-4,
    # with or without dropout; what is under test here is the schedule's way into the net)
    cfg = trainer.TrainConfig(learning_rate=0.0, momentum=0.0, dropout_schedule="0,0.3", dropout_seed=11, total_steps=4)
    tr = trainer.EgsTrainer(_xcfg(), den, max_egs=8, max_frames=1200, config=cfg)
    synth.init_network(tr.net)
    seen = []
    for frac, want in ((0.5, 0.15), (1.0, 0.3), (None, 0.15)):   # None: steps taken (2) / total_steps (4)
        tr.step(batch, fraction=frac)
        r = tr.result()
        assert r.num_ok == batch.batch_size and np.isfinite(r.objf)
        assert all(abs(tr.net.dropout_proportion(n) - want) < 1e-6 for n in TDNNF)
        m = tr.net.dropout_mask("tdnnf6")
        assert m.shape == (batch.batch_size, 256)
        assert m.min() >= 1 - 2 * want - 1e-6 and m.max() <= 1 + 2 * want + 1e-6
        seen.append((m - 1) / (2 * want))
    assert tr.net.dropout_step() == 3
    assert not np.allclose(seen[0], seen[1], atol=1e-3) and not np.allclose(seen[0], seen[2], atol=1e-3)
    # an empty schedule calls nothing: the switch stays off
    tr0 = trainer.EgsTrainer(_xcfg(), den, max_egs=8, max_frames=1200, config=trainer.TrainConfig(learning_rate=0.0))
    synth.init_network(tr0.net)
    tr0.step(batch)
    assert np.isfinite(tr0.result().objf) and tr0.net.dropout_step() == 0
    with pytest.raises(ValueError):
        trainer.EgsTrainer(_xcfg(), den, max_egs=8, max_frames=1200,
                           config=trainer.TrainConfig(dropout_schedule="0,0.9"))
