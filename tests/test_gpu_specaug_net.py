"""SpecAugment at network level (kf_nnet.h nnet_set_spec_augment):
configs/specaug/tiny_specaug.xconfig, T = 200, three sequences of unequal length, m = 10, z = 0.2, f = 0.5.

The masks are integers and the masked activation a select, so those comparisons are bit for
bit. The layers above are compared with the committed CPU oracle, which does not know the
layer: it runs the xconfig from cnn1 upwards on the masked activation read back from the
product. Bounds are test_gpu_dropout_net.py's for the same tensors: activations 2e-3 relative
Frobenius, gradients 5e-3. Observed on an MI355X: activations 6.9e-6 ... 7.3e-4,
gradients 2.0e-5 ... 7.3e-4, full rows and row-subsampled."""
import numpy as np
import pytest

import dropout_ref as dr
import specaug_ref as sr
from conftest import rel_fro

pytestmark = pytest.mark.gpu

SA = "idct-spec-augment"
T, SEQ = 200, [0, 50, 51, 200]
SEED, F, Z_, M = 0x5A5A0123456789AB, 0.5, 0.2, 10
ABOVE = ["cnn1", "cnn2", "cnn3", "cnn4", "tdnnf5", "tdnnf6", "tdnnf7", "tdnnf8", "prefinal-l", "prefinal-chain", "output"]


def _ref_rows(seed, step, seq=SEQ, f=F, z=Z_, m=M, k=0, D=40):
    return sr.specaug_rows(seed, step, k, seq, D, sr.max_bins(D, f), z, m, sr.max_kept(m, z))


def _net(kfp16, xcfg, T=T, seq=SEQ, on=True, seed=SEED):
    from kfp16 import synth
    net = kfp16.Network(xcfg, max_frames=T)
    params, bns = synth.init_network(net)
    if seq is not None:
        net.set_sequences(seq)
    net.set_spec_augment(on, seed)
    return net, params, bns


def _out_grad(T, Pdim, seed=7, rows=None):
    og = (np.random.default_rng(seed).standard_normal((T, Pdim)) * 0.05).astype(np.float16)
    if rows is not None:   # supervised rows only
        z = np.zeros_like(og)
        z[rows] = og[rows]
        og = z
    return og


STRIDE1 = "name=tdnnf8 dim=256 bottleneck-dim=64 time-stride=1"


def _stride3(xcfg):
    """tdnnf8 at time-stride 3, so that the whole TDNN-F stack is part of the compact row set (as
    test_gpu_dropout_net.py does for row subsampling)"""
    assert xcfg.count(STRIDE1) == 1
    return xcfg.replace(STRIDE1, STRIDE1[:-1] + "3")


def _upper_xconfig(xcfg):
    """the xconfig from cnn1 upwards on a 40-dim input: what the oracle runs on the masked activation"""
    lines = [l for l in xcfg.splitlines() if l.strip() and not l.startswith("#")]
    i = [j for j, l in enumerate(lines) if "name=cnn1 " in l][0]
    return "\n".join(["input name=input dim=40"] + lines[i:]) + "\n"


def _run(net, kfp16, fb, gb):
    net.forward(fb.ptr, T)
    out = net.read_activation("output").copy()
    net.backward(gb.ptr)
    return out, net.read_grads()


def test_switch_off_is_the_net_without_the_layer(gpu):
    """off, and on with nothing to draw (f = 0, z = 0): output and gradients of tiny.xconfig with
    the same parameters, bit for bit; the layer's activation is its input's"""
    kfp16 = gpu
    from kfp16 import synth
    fb = kfp16.upload_fp16(synth.make_features(T, 40))
    gb = kfp16.upload_fp16(_out_grad(T, 200))
    plain, _, _ = _net(kfp16, synth.load_xconfig("tiny.xconfig"), on=False)
    o0, g0 = _run(plain, kfp16, fb, gb)
    plain.close()
    net, _, _ = _net(kfp16, synth.load_xconfig("specaug/tiny_specaug.xconfig"), on=False)
    o1, g1 = _run(net, kfp16, fb, gb)
    assert net.spec_augment_step() == 0                      # off: the step does not advance
    with pytest.raises(kfp16.KfError, match="no mask"):
        net.spec_augment_rows(SA)
    assert net.activation(SA)[0] == net.activation("idct-batchnorm")[0]    # the alias
    net.set_spec_augment(True, SEED)
    o2, g2 = _run(net, kfp16, fb, gb)                        # on: differs
    assert net.spec_augment_step() == 1 and not np.array_equal(o2, o0)
    assert net.activation(SA)[0] != net.activation("idct-batchnorm")[0]
    net.set_spec_augment_opts(SA, 0.0, 0.0, M)
    o3, g3 = _run(net, kfp16, fb, gb)                        # on, nothing to draw: the step advances
    assert net.spec_augment_step() == 2
    with pytest.raises(kfp16.KfError, match="no mask"):
        net.spec_augment_rows(SA)
    net.set_spec_augment_opts(SA, F, Z_, M)
    net.set_spec_augment(False)
    o4, g4 = _run(net, kfp16, fb, gb)                        # off after on
    for o, g in ((o1, g1), (o3, g3), (o4, g4)):
        assert np.array_equal(o.view(np.uint16), o0.view(np.uint16))
        assert set(g) == set(g0)
        for k in g0:
            assert np.array_equal(g[k], g0[k]), k
    net.close()


@pytest.mark.parametrize("sub", [False, True], ids=["full-rows", "row-subsampling"])
def test_switch_on_against_reference(gpu, sub):
    kfp16 = gpu
    import oracle
    from kfp16 import synth
    xcfg = synth.load_xconfig("specaug/tiny_specaug.xconfig")
    if sub:
        xcfg = _stride3(xcfg)
    upper = _upper_xconfig(xcfg)
    assert "spec-augment" not in upper and upper.count("\n") == 12
    net, params, bns = _net(kfp16, xcfg)
    if sub:
        net.set_row_subsampling(3)
    assert net.spec_augment_layers() == [SA]
    feats = synth.make_features(T, 40)
    fb = kfp16.upload_fp16(feats)
    net.forward(fb.ptr, T)
    tc, tc0, rows = net.row_set()
    assert (tc > 0) == sub, "the row set was not used: T too small for its guard"
    assert net.spec_augment_step() == 1
    rb = net.spec_augment_rows(SA)
    ref_rb = _ref_rows(SEED, 0)
    assert rb.dtype == np.int32 and np.array_equal(rb, ref_rb)
    assert np.any(rb == -1) and np.any(rb != -1)
    x_in = net.read_activation("idct-batchnorm")
    x_sa = net.read_activation(SA)
    assert x_sa.shape == (T, 40)
    assert np.array_equal(x_sa.view(np.uint16), sr.specaug_apply(x_in, rb).view(np.uint16))
    assert not np.array_equal(x_sa.view(np.uint16), x_in.view(np.uint16))
    # the layers above, against the oracle on the masked activation
    tp = {k: synth.trunc_fp16(v) for k, v in params.items()}
    on = oracle.OracleNet(upper, tp, bns, round_mode=oracle.ROUND_FUSED, threads=16)
    on.forward(x_sa.astype(np.float32))
    for name in ABOVE:
        got, ref = net.read_activation(name).astype(np.float32), on.act(name)
        if got.shape[0] != T:                                # compact rows (row subsampling): frames 3c
            assert sub and got.shape[0] == tc
            got, ref = got[:tc0], ref[rows[:tc0]]
        e = rel_fro(got, ref)
        print("%s: rel fro %.2e" % (name, e))
        assert e <= 2e-3, (name, e)
    # the masks did something: the oracle on the unmasked input is far from the product
    off = oracle.OracleNet(upper, tp, bns, round_mode=oracle.ROUND_FUSED, threads=16)
    off.forward(x_in.astype(np.float32))
    assert rel_fro(net.read_activation("cnn1").astype(np.float32), off.act("cnn1")) > 0.05
    off.close()
    # backward with the product's ReLU decisions replayed, as test_gpu_nnet.py does
    # (with row subsampling the decisions of a full-rows forward of the same (seed, step): the rows
    # of the set are bit-identical to it, test_gpu_row_subsampling.py, and the oracle needs all rows)
    if sub:
        full, _, _ = _net(kfp16, xcfg)
        full.forward(fb.ptr, T)
        assert np.array_equal(full.spec_augment_rows(SA), rb)
        relu = full.relu_masks()
        full.close()
    else:
        relu = net.relu_masks()
    on.forward(x_sa.astype(np.float32), force_masks={k: v for k, v in relu.items() if k in ABOVE})
    sup = np.arange(30, T, 3)
    og = _out_grad(T, 200, rows=sup)
    gb = kfp16.upload_fp16(og[rows] if sub else og)
    net.backward(gb.ptr)
    got = net.read_grads()
    ref = on.backward(og.astype(np.float32)) or on.grads()
    errs = {k: rel_fro(got[k], ref[k]) for k in ref}
    print("grad errors: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert set(errs) == set(got) and "cnn1.W" in errs       # cnn1's weight gradient reads the masked input
    bad = {k: v for k, v in errs.items() if v > 5e-3}
    assert not bad, bad
    # ... and not the unmasked one: cnn1.W's gradient with the switch off is far away
    net.set_spec_augment(False)
    net.forward(fb.ptr, T)
    net.backward(gb.ptr)
    assert rel_fro(net.read_grads()["cnn1.W"], ref["cnn1.W"]) > 0.05
    on.close()
    net.close()


def test_replay_and_steps(gpu):
    kfp16 = gpu
    from kfp16 import synth
    fb = kfp16.upload_fp16(synth.make_features(T, 40))
    gb = kfp16.upload_fp16(_out_grad(T, 200))
    net, _, _ = _net(kfp16, synth.load_xconfig("specaug/tiny_specaug.xconfig"))
    o0, g0 = _run(net, kfp16, fb, gb)
    r0 = net.spec_augment_rows(SA)
    o1, _ = _run(net, kfp16, fb, gb)                         # step 1: other rows
    r1 = net.spec_augment_rows(SA)
    assert net.spec_augment_step() == 2
    assert not np.array_equal(r0, r1) and np.array_equal(r1, _ref_rows(SEED, 1)) and not np.array_equal(o0, o1)
    net.set_spec_augment_step(0)
    net.set_wgrad_stream(False)
    o2, g2 = _run(net, kfp16, fb, gb)                        # replay of step 0
    net.set_wgrad_stream(True)
    assert np.array_equal(net.spec_augment_rows(SA), r0)
    assert np.array_equal(o2.view(np.uint16), o0.view(np.uint16)) and all(np.array_equal(g2[k], g0[k]) for k in g0)
    net.set_spec_augment_step(2 ** 32 - 1)                   # the step wraps at 2^32
    net.forward(fb.ptr, T)
    assert net.spec_augment_step() == 0
    assert np.array_equal(net.spec_augment_rows(SA), _ref_rows(SEED, 2 ** 32 - 1))
    net.set_spec_augment(True, SEED + 1)                     # another seed
    net.set_spec_augment_step(0)
    net.forward(fb.ptr, T)
    assert np.array_equal(net.spec_augment_rows(SA), _ref_rows(SEED + 1, 0)) and not np.array_equal(net.spec_augment_rows(SA), r0)
    # other options reach the kernel; z = 0 leaves the band only
    net.set_spec_augment_opts(SA, 1.0, 0.0, 3)
    net.set_spec_augment_step(4)
    net.forward(fb.ptr, T)
    rb = net.spec_augment_rows(SA)
    assert np.array_equal(rb, _ref_rows(SEED + 1, 4, f=1.0, z=0.0, m=3)) and not np.any(rb == -1)
    net.set_spec_augment_opts(SA, 0.0, 0.5, 2)
    net.set_spec_augment_step(4)
    net.forward(fb.ptr, T)
    assert np.array_equal(net.spec_augment_rows(SA), _ref_rows(SEED + 1, 4, f=0.0, z=0.5, m=2))
    # a forward whose T is not the boundaries' fails while the switch is on
    with pytest.raises(kfp16.KfError, match="nnet_set_sequences"):
        net.forward(fb.ptr, T - 1)
    net.set_sequences(None)                                  # one sequence
    net.set_spec_augment_step(9)
    net.forward(fb.ptr, T - 1)
    assert np.array_equal(net.spec_augment_rows(SA), _ref_rows(SEED + 1, 9, seq=[0, T - 1], f=0.0, z=0.5, m=2))
    net.close()


def test_with_dropout_natural_gradient_and_implicit_dz(gpu):
    """dropout on as well: both masks equal their references (their streams do not meet); NG-SGD
    and implicit dz run with the switch on"""
    kfp16 = gpu
    from kfp16 import synth
    xcfg = synth.load_xconfig("specaug/tiny_specaug.xconfig")
    assert xcfg.count("bypass-scale=0.66") == 4
    xd = xcfg.replace("bypass-scale=0.66", "bypass-scale=0.66 dropout-proportion=0.3")
    fb = kfp16.upload_fp16(synth.make_features(T, 40))
    gb = kfp16.upload_fp16(_out_grad(T, 200))
    net, _, _ = _net(kfp16, xd)
    net.set_dropout(True, SEED)                              # the same seed: the high counter bit separates the streams
    net.set_natural_gradient(True)
    net.forward(fb.ptr, T)
    net.forward(fb.ptr, T)
    assert net.dropout_step() == 2 and net.spec_augment_step() == 2
    assert np.array_equal(net.spec_augment_rows(SA), _ref_rows(SEED, 1))
    for i, n in enumerate(net.dropout_layers()):
        got, ref = net.dropout_mask(n), dr.dropout_masks(SEED, 1, i, len(SEQ) - 1, 256, 0.3)
        assert np.all(np.abs(got - ref) <= np.spacing(np.maximum(np.abs(ref), np.abs(got)))), n
    x_in, x_sa = net.read_activation("idct-batchnorm"), net.read_activation(SA)
    assert np.array_equal(x_sa.view(np.uint16), sr.specaug_apply(x_in, net.spec_augment_rows(SA)).view(np.uint16))
    net.backward(gb.ptr)
    stats = net.natural_gradient_stats()
    assert stats and not any(s["flag"] for s in stats)
    g = net.read_grads()
    assert all(np.isfinite(v).all() for v in g.values()) and np.abs(g["cnn1.W"]).max() > 0
    net.close()
    # implicit dz with the switch on: the same masked activation, finite gradients
    net, _, _ = _net(kfp16, xcfg)
    net.set_implicit_dz(True)
    o, g = _run(net, kfp16, fb, gb)
    assert np.array_equal(net.spec_augment_rows(SA), _ref_rows(SEED, 0))
    assert np.isfinite(o.astype(np.float32)).all() and all(np.isfinite(v).all() for v in g.values())
    net.close()


def test_ivector_front_end(gpu):
    """tiny_ivec_specaug.xconfig: the layer's activation is masked and combine_inputs carries the
    masked values in its feature filter (filter 0 of 6 per height); the ivector filters do not change"""
    kf = gpu
    from kfp16 import synth
    Ti, seq = 150, np.array([0, 40, 97, 150], np.int32)
    net = kf.Network(synth.load_xconfig("specaug/tiny_ivec_specaug.xconfig"), max_frames=Ti)
    synth.init_network(net)
    rng = np.random.default_rng(5)
    ivec = (rng.standard_normal((3, 100)) * 2).astype(np.float16)
    fb, ib = kf.upload_fp16(synth.make_features(Ti, 40)), kf.upload_fp16(ivec)
    net.forward_ivector(fb.ptr, Ti, ib.ptr, seq)
    c0 = net.read_activation("combine_inputs").reshape(Ti, 40, 6)
    net.set_spec_augment(True, SEED)
    net.forward_ivector(fb.ptr, Ti, ib.ptr, seq)
    rb = net.spec_augment_rows(SA)
    assert np.array_equal(rb, _ref_rows(SEED, 0, seq=seq))
    x_in, x_sa = net.read_activation("idct-batchnorm"), net.read_activation(SA)
    want = sr.specaug_apply(x_in, rb)
    assert np.array_equal(x_sa.view(np.uint16), want.view(np.uint16)) and not np.array_equal(want.view(np.uint16), x_in.view(np.uint16))
    c1 = net.read_activation("combine_inputs").reshape(Ti, 40, 6)
    assert np.array_equal(c1[:, :, 0].view(np.uint16), want.view(np.uint16))
    assert np.array_equal(c0[:, :, 0].view(np.uint16), x_in.view(np.uint16))
    assert np.array_equal(c1[:, :, 1:].view(np.uint16), c0[:, :, 1:].view(np.uint16))
    gb = kf.upload_fp16(_out_grad(Ti, 200))
    net.backward(gb.ptr)                                     # reaches ivector-linear through the combine
    g = net.read_grads()
    assert all(np.isfinite(v).all() for v in g.values()) and np.abs(g["ivector-linear.W"]).sum() > 0
    net.close()


def test_trainer(gpu, tmp_path):
    """EgsTrainer with spec_augment=True on the egs fixture of test_gpu_egs_train.py: two steps run,
    one sequence per eg, the rows differ between the steps and between ranks 0 and 1"""
    kf = gpu
    import egs_writer as W
    from kfp16 import egs, synth, trainer
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, 6, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=6).next_batch()
    den = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)
    xcfg = synth.load_xconfig("specaug/tiny_specaug.xconfig")
    seq = np.append(np.asarray(batch.frame_offsets, np.int64), batch.total_frames)
    seen = {}
    for rank in (0, 1):
        cfg = trainer.TrainConfig(learning_rate=0.0, momentum=0.0, spec_augment=True, spec_augment_seed=11)
        tr = trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=1200, config=cfg, rank=rank)
        synth.init_network(tr.net)
        for step in range(2 if rank == 0 else 1):
            tr.step(batch)
            r = tr.result()
            assert r.num_ok == batch.batch_size and np.isfinite(r.objf)
            rb = tr.net.spec_augment_rows(SA)
            seed = (11 + 0x9E3779B97F4A7C15 * rank) % 2 ** 64
            assert np.array_equal(rb, _ref_rows(seed, step, seq=seq))      # one sequence per eg
            seen[(rank, step)] = rb
        assert tr.net.spec_augment_step() == (2 if rank == 0 else 1)
    assert not np.array_equal(seen[(0, 0)], seen[(0, 1)]) and not np.array_equal(seen[(0, 0)], seen[(1, 0)])
    tr0 = trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=1200, config=trainer.TrainConfig(learning_rate=0.0))
    synth.init_network(tr0.net)
    tr0.step(batch)                                          # the default: the switch stays off
    assert np.isfinite(tr0.result().objf) and tr0.net.spec_augment_step() == 0


def test_mxfp8_conflict_and_fp8_without_one(gpu):
    kfp16 = gpu
    from kfp16 import synth
    fb = kfp16.upload_fp16(synth.make_features(T, 40))
    # a spec-augment layer between tdnnf8 and prefinal-l: prefinal-l would read tdnnf8's MXFP8 copy
    x = synth.load_xconfig("tiny.xconfig").replace("linear-component name=prefinal-l dim=64",
                                                   "spec-augment-layer name=sa2\nlinear-component name=prefinal-l dim=64")
    net, _, _ = _net(kfp16, x, on=True)
    with pytest.raises(kfp16.KfError, match="MXFP8 copy"):
        net.set_fp8(True)
    net.set_spec_augment(False)
    net.set_fp8(True)
    with pytest.raises(kfp16.KfError, match="MXFP8 copy"):
        net.set_spec_augment(True, SEED)
    net.forward(fb.ptr, T)                                   # the net still works, SpecAugment off
    net.set_fp8(False)
    net.set_spec_augment(True, SEED)
    net.forward(fb.ptr, T)
    assert np.array_equal(net.spec_augment_rows("sa2"), _ref_rows(SEED, 0, D=256))
    net.close()
    # tiny_specaug.xconfig: the layer's consumer is a conv, which reads fp16: MXFP8 mode is fine
    net, _, _ = _net(kfp16, synth.load_xconfig("specaug/tiny_specaug.xconfig"))
    net.set_fp8(True)
    net.forward(fb.ptr, T)
    rb = net.spec_augment_rows(SA)
    assert np.array_equal(rb, _ref_rows(SEED, 0))
    assert np.array_equal(net.read_activation(SA).view(np.uint16),
                          sr.specaug_apply(net.read_activation("idct-batchnorm"), rb).view(np.uint16))
    assert np.isfinite(net.read_activation("output").astype(np.float32)).all()
    net.close()
