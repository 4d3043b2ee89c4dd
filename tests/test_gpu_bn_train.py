"""Training-mode BatchNorm of the TDNN-F layers (kf_ops.h kf_bn_train_*, kf_nnet.h
nnet_set_bn_train): the four kernels against float64, then the network on
configs/tiny.xconfig (300 frames, 3 sequences) against the staged reference
(tests/bn_train_ref.py BnTrainOracle). Network tolerances are test_gpu_nnet.py's for the same
tensors: activations 2e-3 relative Frobenius and 1e-2 of the largest value, gradients 5e-3."""
import numpy as np
import pytest

import bn_train_ref as br
from conftest import max_abs_rel, rel_fro

pytestmark = pytest.mark.gpu

TDNNF = ["tdnnf5", "tdnnf6", "tdnnf7", "tdnnf8"]
T = 300
SEQ = [0, 90, 200, 300]
EPS = 1e-3
U24, U23 = 2.0 ** -24, 2.0 ** -23

# rows: one, a few past the 4 row lanes, one past a chunk of 256, a few past four chunks;
# D: one lane, part of a slab of 512, three slabs; one case with ld > D
SHAPES = [(rows, D, D) for rows in (1, 7, 257, 1031) for D in (8, 160, 1536)] + [(257, 160, 192)]


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------
def _r_matrix(rng, rows, D):
    """a ReLU output in fp16 with the columns that break naive sums: 0 all zero, 1 constant
    (var 0), 2 mean 4 with standard deviation 1/64"""
    r = np.maximum(rng.standard_normal((rows, D)) + 0.3, 0.0)
    r[:, 0] = 0.0
    r[:, 1] = 2.5
    r[:, 2] = 4.0 + rng.standard_normal(rows) / 64.0
    return r.astype(np.float16)


def _pad(a, ld, fill=0):
    out = np.full((a.shape[0], ld), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _f16_ulp(x):
    return np.maximum(np.spacing(np.abs(x).astype(np.float16)).astype(np.float64), 2.0 ** -24)


def _read_f64(kf, buf, n):
    return kf.read_f32(buf.ptr, (2 * n,)).view(np.float64).copy()


def _fwd_kernels(kf, r16, ld, rms, drop, seg, x16, alpha, acc=None):
    rows, D = r16.shape
    rb = kf.upload_fp16(_pad(r16, ld, 7))                 # (the pad columns must not be read)
    st = kf.upload_f32(np.zeros(4 * D, np.float32))
    p = lambda k: st.ptr + 4 * D * k
    ap = (acc.ptr, acc.ptr + 16, acc.ptr + 16 + 8 * D) if acc is not None else (None, None, None)
    kf.check(kf.core.kf_bn_train_stats(rb.ptr, ld, rows, D, EPS, rms, p(0), p(1), p(2), p(3), *ap), "kf_bn_train_stats")
    ob = kf.upload_fp16(np.full((rows, ld), 9, np.float16))
    db = kf.upload_f32(drop) if drop is not None else None
    sb = kf.upload_f32(np.asarray(seg, np.int32).view(np.float32)) if drop is not None else None
    xb = kf.upload_fp16(_pad(x16, ld)) if x16 is not None else None
    kf.check(kf.core.kf_bn_train_apply(rb.ptr, ld, rows, D, p(2), p(3), db.ptr if db else None, D, sb.ptr if sb else None,
                                       xb.ptr if xb else None, ld, alpha, ob.ptr, ld), "kf_bn_train_apply")
    stats = kf.read_f32(st.ptr, (4, D))
    out = kf.read_fp16(ob.ptr, (rows, ld))
    return stats, out


@pytest.mark.parametrize("rows,D,ld", SHAPES)
def test_forward_kernels_against_float64(gpu, rows, D, ld):
    kf = gpu
    rng = np.random.default_rng(rows * 7 + D)
    rms, alpha = 0.75, 0.66
    r16 = _r_matrix(rng, rows, D)
    x16 = rng.standard_normal((rows, D)).astype(np.float16)
    seg = (np.arange(rows) * 3) // rows
    drop = rng.uniform(0.4, 1.6, size=(3, D)).astype(np.float32)
    r, x = r16.astype(np.float64), x16.astype(np.float64)
    ref = br.bn_train_forward(r, EPS, rms, drop, seg, x, alpha)
    acc = kf.upload_f32(np.zeros(2 * (2 + 2 * D), np.float32))
    stats, out = _fwd_kernels(kf, r16, ld, rms, drop, seg, x16, alpha, acc)
    mean, var, scale, shift = (s.astype(np.float64) for s in stats)
    er2 = (r * r).mean(0)
    # fp32 storage of a double result: half an fp32 ulp each, the double sums' own error (n 2^-53
    # relative on sum r and sum r^2) far below the 1e-12 E[r^2] term
    print("mean err / bound %.3g" % np.max(np.abs(mean - ref["mean"]) / (U23 * np.abs(ref["mean"]) + 1e-300)))
    assert np.all(np.abs(mean - ref["mean"]) <= U23 * np.abs(ref["mean"]))
    bvar = U23 * ref["var"] + 1e-12 * er2
    assert np.all(np.abs(var - ref["var"]) <= bvar)
    assert var[0] == 0.0 and var[1] == 0.0 and np.all(var >= 0)
    # scale = rms (var + eps)^-1/2: d scale = scale / 2 * d var / (var + eps), plus its own storage
    bsc = U23 * ref["scale"] + 0.5 * ref["scale"] * (1e-12 * er2) / (ref["var"] + EPS)
    assert np.all(np.abs(scale - ref["scale"]) <= bsc)
    bsh = U23 * np.abs(ref["shift"]) + np.abs(ref["mean"]) * bsc
    assert np.all(np.abs(shift - ref["shift"]) <= bsh)
    # out: one fp16 ulp, the statistics' error carried through (|r| d scale + d shift) |drop|, and
    # the three fp32 roundings of the epilogue's fmaf, multiply, fmaf
    d = drop[seg].astype(np.float64)
    mag = (np.abs(r * ref["scale"]) + np.abs(ref["shift"])) * d
    tol = _f16_ulp(ref["out"]) + (np.abs(r) * bsc + bsh) * d + 3 * U24 * (mag + np.abs(alpha * x))
    err = np.abs(out[:, :D].astype(np.float64) - ref["out"])
    print("out err / tol max %.3g" % np.max(err / tol))
    assert np.all(err <= tol)
    assert np.all(out[:, D:] == 9)                        # nothing past D is written
    # the accumulators took this batch
    a = _read_f64(kf, acc, 2 + 2 * D)
    assert a[0] == rows
    assert np.all(np.abs(a[2:2 + D] - r.sum(0)) <= 1e-12 * np.abs(r).sum(0))
    assert np.all(np.abs(a[2 + D:] - (r * r).sum(0)) <= 1e-12 * (r * r).sum(0))
    # bit for bit on a second run
    stats2, out2 = _fwd_kernels(kf, r16, ld, rms, drop, seg, x16, alpha, acc)
    assert np.array_equal(stats.view(np.uint32), stats2.view(np.uint32))
    assert np.array_equal(out.view(np.uint16), out2.view(np.uint16))
    assert _read_f64(kf, acc, 2 + 2 * D)[0] == 2 * rows
    # without dropout and bypass: the constant and zero columns come out as 0 + shift + r scale
    stats3, out3 = _fwd_kernels(kf, r16, ld, rms, None, None, None, 0.0)
    ref3 = br.bn_train_forward(r, EPS, rms)
    assert np.array_equal(stats3.view(np.uint32), stats.view(np.uint32))
    tol3 = _f16_ulp(ref3["out"]) + np.abs(r) * bsc + bsh + 3 * U24 * (np.abs(r * ref["scale"]) + np.abs(ref["shift"]))
    assert np.all(np.abs(out3[:, :D].astype(np.float64) - ref3["out"]) <= tol3)


@pytest.mark.parametrize("with_drop", [False, True])
@pytest.mark.parametrize("rows,D,ld", SHAPES)
def test_backward_kernels_against_float64(gpu, rows, D, ld, with_drop):
    kf = gpu
    rng = np.random.default_rng(rows * 11 + D + with_drop)
    rms = 0.75
    r16 = _r_matrix(rng, rows, D)
    g16 = (rng.standard_normal((rows, D)) * 0.1).astype(np.float16)
    r, g = r16.astype(np.float64), g16.astype(np.float64)
    fwd = br.bn_train_forward(r, EPS, rms)
    sc32, sh32 = fwd["scale"].astype(np.float32), fwd["shift"].astype(np.float32)
    seg = (np.arange(rows) * 3) // rows
    drop = rng.uniform(0.4, 1.6, size=(3, D)).astype(np.float32) if with_drop else None
    bits = rng.integers(0, 2, size=(rows, D)).astype(np.uint8)
    packed = np.packbits(bits.reshape(-1), bitorder="little")
    # the reference on the kernel's inputs: the fp32 scale and shift it is handed
    sc, sh = sc32.astype(np.float64), sh32.astype(np.float64)
    a_ref, b_ref, gr = br.bn_train_backward(g, r, sc, sh, rms, drop, seg if with_drop else None)
    dz_ref = gr * bits

    gb, rb = kf.upload_fp16(_pad(g16, ld, 5)), kf.upload_fp16(_pad(r16, ld, 7))
    scb, shb = kf.upload_f32(sc32), kf.upload_f32(sh32)
    ab = kf.upload_f32(np.zeros(2 * D, np.float32))
    db = kf.upload_f32(drop) if with_drop else None
    sb = kf.upload_f32(seg.astype(np.int32).view(np.float32)) if with_drop else None
    mb = kf.upload_f32(np.frombuffer(packed.tobytes() + b"\0" * (-len(packed) % 4), np.float32))
    dzb = kf.upload_fp16(np.full((rows, ld), 9, np.float16))
    dp, sp = (db.ptr, sb.ptr) if with_drop else (None, None)

    def run():
        kf.check(kf.core.kf_bn_train_bwd_stats(gb.ptr, ld, rb.ptr, ld, rows, D, scb.ptr, shb.ptr, rms, dp, D, sp, ab.ptr,
                                               ab.ptr + 4 * D), "kf_bn_train_bwd_stats")
        kf.check(kf.core.kf_bn_train_bwd_apply(gb.ptr, ld, rb.ptr, ld, rows, D, scb.ptr, shb.ptr, rms, ab.ptr, ab.ptr + 4 * D,
                                               dp, D, sp, mb.ptr, D, dzb.ptr, ld), "kf_bn_train_bwd_apply")
        return kf.read_f32(ab.ptr, (2, D)), kf.read_fp16(dzb.ptr, (rows, ld))

    ab1, dz1 = run()
    a, b = ab1[0].astype(np.float64), ab1[1].astype(np.float64)
    dy = g * (drop[seg].astype(np.float64) if with_drop else 1.0)
    # fp32 storage of double sums. b = (scale sum dy r + shift sum dy) / (rms n) cancels where the
    # column's mean is far above its deviation: the absolute term is on the terms' magnitudes
    ba = U23 * np.abs(a_ref) + 1e-12 * np.abs(dy).mean(0)
    bb = U23 * np.abs(b_ref) + 1e-12 * (np.abs(sc) * np.abs(dy * r).mean(0) + np.abs(sh) * np.abs(dy).mean(0)) / rms
    assert np.all(np.abs(a - a_ref) <= ba)
    assert np.all(np.abs(b - b_ref) <= bb)
    yhat = (r * sc + sh) / rms
    tol = _f16_ulp(dz_ref) + np.abs(sc) * (ba + np.abs(yhat) * bb)
    err = np.abs(dz1[:, :D].astype(np.float64) - dz_ref)
    print("dz err / tol max %.3g" % np.max(err / tol))
    assert np.all(err <= tol)
    assert np.all(dz1[:, :D][bits == 0] == 0)
    assert np.all(dz1[:, D:] == 9)
    ab2, dz2 = run()
    assert np.array_equal(ab1.view(np.uint32), ab2.view(np.uint32)) and np.array_equal(dz1.view(np.uint16), dz2.view(np.uint16))


def test_kernel_argument_checks(gpu):
    kf = gpu
    buf = kf.upload_f32(np.zeros(64, np.float32))
    p = buf.ptr
    assert kf.core.kf_bn_train_stats(p, 12, 4, 12, EPS, 1.0, p, p, p, p, None, None, None) != 0      # D % 8
    assert kf.core.kf_bn_train_stats(p, 8, 4, 16, EPS, 1.0, p, p, p, p, None, None, None) != 0       # ld < D
    assert kf.core.kf_bn_train_stats(p, 8, 0, 8, EPS, 1.0, p, p, p, p, None, None, None) != 0        # rows
    assert kf.core.kf_bn_train_stats(p, 8, 4, 8, EPS, 1.0, p, p, p, p, p, None, None) != 0           # one accumulator
    assert kf.core.kf_bn_train_apply(p, 8, 4, 8, p, p, p, 8, None, None, 0, 0.0, p, 8) != 0           # drop without row_seg
    assert b"kf_bn_train" in kf.core.kf_last_error()


# ---------------------------------------------------------------------------
# network
# ---------------------------------------------------------------------------
def _xcfg(dropout=False):
    from kfp16 import synth
    x = synth.load_xconfig("tiny.xconfig")
    assert x.count("bypass-scale=0.66") == 4
    return x.replace("bypass-scale=0.66", "bypass-scale=0.66 dropout-proportion=0.0") if dropout else x


def _features(seed=1234, frames=T):
    from kfp16 import synth
    return synth.make_features(frames, 40, seed=seed)


def _out_grad(frames=T, seed=7):
    return (np.random.default_rng(seed).standard_normal((frames, 200)) * 0.05).astype(np.float16)


def _net(kf, xcfg, seq=SEQ):
    from kfp16 import synth
    net = kf.Network(xcfg, max_frames=T)
    params, bns = synth.init_network(net)
    if seq is not None:
        net.set_sequences(seq)
    return net, params, bns


def _run(net, fb, gb, frames=T):
    net.forward(fb.ptr, frames)
    out = net.read_activation("output").copy()
    net.backward(gb.ptr)
    return out, net.read_grads()


def _reference_run(kf, dropout):
    """One train-mode forward / backward of tiny on the GPU and the staged reference of it (the
    GPU's ReLU decisions, and its dropout masks, replayed), shared by the tests below."""
    from kfp16 import synth
    xcfg = _xcfg(dropout)
    net, params, bns = _net(kf, xcfg)
    assert net.batchnorm_train_layers() == TDNNF
    net.set_batchnorm_train(True)
    if dropout:
        net.set_dropout_proportion(0.3)
        net.set_dropout(True, 0x5EED5EED12345678)
    feats, og = _features(), _out_grad()
    fb, gb = kf.upload_fp16(feats), kf.upload_fp16(og)
    net.forward(fb.ptr, T)
    names = TDNNF + ["prefinal-l", "prefinal-chain", "output"]
    acts = {n: net.read_activation(n).astype(np.float32) for n in ["cnn4"] + names}
    stats = {n: net.batchnorm_batch_stats(n) for n in TDNNF}
    masks = {n: net.dropout_mask(n) for n in TDNNF} if dropout else None
    relu = net.relu_masks()
    net.backward(gb.ptr)
    grads = net.read_grads()
    net.close()
    tp = {k: synth.trunc_fp16(v) for k, v in params.items()}
    on = br.BnTrainOracle(xcfg, tp, bns, TDNNF, masks=masks, seq_row0=SEQ, threads=16)
    on.forward(feats.astype(np.float32))
    ref_acts = {n: on.act(n) for n in names}
    ref_stats = dict(on.stats)
    on.forward(feats.astype(np.float32), force_masks=relu)
    ref_grads = on.backward(og.astype(np.float32))
    on.close()
    return dict(xcfg=xcfg, tp=tp, bns=bns, feats=feats, og=og, relu=relu, acts=acts, stats=stats, grads=grads,
                ref_acts=ref_acts, ref_stats=ref_stats, ref_grads=ref_grads, names=names)


@pytest.fixture(scope="module")
def plain_run(gpu):
    import oracle  # noqa: F401  (BnTrainOracle imports it)
    return _reference_run(gpu, dropout=False)


@pytest.fixture(scope="module")
def dropout_run(gpu):
    import oracle  # noqa: F401
    return _reference_run(gpu, dropout=True)


def _check_forward(run):
    for name in run["names"]:
        got, ref = run["acts"][name], run["ref_acts"][name]
        print("%s: rel fro %.2e, max abs rel %.2e" % (name, rel_fro(got, ref), max_abs_rel(got, ref)))
        assert rel_fro(got, ref) <= 2e-3, (name, rel_fro(got, ref))
        assert max_abs_rel(got, ref) <= 1e-2, (name, max_abs_rel(got, ref))
    for name in TDNNF:
        (m, v), (mr, vr) = run["stats"][name], run["ref_stats"][name]
        print("%s: mean rel fro %.2e, var rel fro %.2e" % (name, rel_fro(m, mr), rel_fro(v, vr)))
        assert rel_fro(m, mr) <= 2e-3 and rel_fro(v, vr) <= 2e-3, name


def _check_backward(run):
    got, ref = run["grads"], run["ref_grads"]
    errs = {k: rel_fro(got[k], ref[k]) for k in ref}
    print("grad errors: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert set(errs) == set(got)
    bad = {k: v for k, v in errs.items() if v > 5e-3}
    assert not bad, bad


def test_network_forward(plain_run):
    _check_forward(plain_run)
    # what the normalisation promises, on the layer's own output: the BatchNorm part of a bypass
    # layer has column mean 0 and mean square rms^2 var / (var + eps) (target_rms = 1)
    for name, below in (("tdnnf6", "tdnnf5"), ("tdnnf7", "tdnnf6"), ("tdnnf8", "tdnnf7")):
        y = plain_run["acts"][name].astype(np.float64) - 0.66 * plain_run["acts"][below].astype(np.float64)
        var = plain_run["stats"][name][1].astype(np.float64)
        print("%s: max |column mean| %.2e" % (name, np.abs(y.mean(0)).max()))
        assert np.abs(y.mean(0)).max() <= 2.0 ** -10
        want = var / (var + EPS)
        assert np.all(np.abs((y * y).mean(0) - want) <= 1e-2 * np.maximum(want, 1e-3))


def test_network_backward(plain_run):
    import oracle
    run = plain_run
    _check_backward(run)
    # the feature against its absence: the frozen-statistics gradient (the plain oracle fed the
    # batch statistics, the same ReLU decisions) is far from the train-mode reference on every
    # TDNN-F affine weight, more than 5 x the bound above
    bns = dict(run["bns"])
    for n in TDNNF:
        m, v = run["ref_stats"][n]
        d = m.size
        bns[(n, 0)] = (m.astype(np.float32), v.astype(np.float32), np.ones(d, np.float32), np.zeros(d, np.float32))
    on = oracle.OracleNet(run["xcfg"], run["tp"], bns, round_mode=oracle.ROUND_FUSED, threads=16)
    on.forward(run["feats"].astype(np.float32), force_masks=run["relu"])
    on.backward(run["og"].astype(np.float32))
    frozen = on.grads()
    on.close()
    for n in TDNNF:
        sep = rel_fro(frozen[n + ".AffineW"], run["ref_grads"][n + ".AffineW"])
        print("%s.AffineW: frozen-statistics gradient differs by %.2e" % (n, sep))
        assert sep > 5 * 5e-3, (n, sep)
        assert rel_fro(run["grads"][n + ".AffineW"], frozen[n + ".AffineW"]) > 4 * 5e-3, n


def test_network_with_dropout(dropout_run):
    _check_forward(dropout_run)
    _check_backward(dropout_run)


def test_mode_hygiene(gpu):
    """the mode leaves nothing behind: outputs and gradients before it was ever on equal those
    after on -> forward -> backward -> off, bit for bit; two train-mode steps on one input agree
    bit for bit, with the weight gradients on their own stream or not"""
    kf = gpu
    net, _, _ = _net(kf, _xcfg())
    fb, gb = kf.upload_fp16(_features()), kf.upload_fp16(_out_grad())
    o0, g0 = _run(net, fb, gb)
    with pytest.raises(kf.KfError, match="training mode"):
        net.batchnorm_batch_stats("tdnnf6")
    net.set_batchnorm_train(True)
    o1, g1 = _run(net, fb, gb)
    s1 = net.batchnorm_batch_stats("tdnnf7")
    assert not np.array_equal(o1, o0)
    o2, g2 = _run(net, fb, gb)
    net.set_wgrad_stream(False)
    o3, g3 = _run(net, fb, gb)
    net.set_wgrad_stream(True)
    s3 = net.batchnorm_batch_stats("tdnnf7")
    for o, g in ((o2, g2), (o3, g3)):
        assert np.array_equal(o.view(np.uint16), o1.view(np.uint16))
        for k in g1:
            assert np.array_equal(g[k].view(np.uint32), g1[k].view(np.uint32)), k
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(s1, s3))
    net.set_batchnorm_train(False)
    o4, g4 = _run(net, fb, gb)
    assert np.array_equal(o4.view(np.uint16), o0.view(np.uint16))
    for k in g0:
        assert np.array_equal(g4[k].view(np.uint32), g0[k].view(np.uint32)), k
    with pytest.raises(kf.KfError, match="does not govern"):
        net.batchnorm_batch_stats("prefinal-chain", 1)
    net.close()


def test_accumulators_and_commit(gpu):
    kf = gpu
    import oracle
    from kfp16 import synth
    xcfg = _xcfg()
    net, params, bns = _net(kf, xcfg, seq=None)
    net.set_batchnorm_train(True)
    net.batchnorm_zero_stats()
    fa, fb2 = _features(), _features(seed=99, frames=210)
    ba, bb = kf.upload_fp16(fa), kf.upload_fp16(fb2)
    want = {n: [0.0, 0.0] for n in TDNNF}
    for buf, frames in ((ba, 300), (bb, 210)):
        net.forward(buf.ptr, frames)
        for n in TDNNF:
            m, v = (s.astype(np.float64) for s in net.batchnorm_batch_stats(n))
            want[n][0] = want[n][0] + frames * m
            want[n][1] = want[n][1] + frames * (v + m * m)
    pooled = {}
    for n in TDNNF:
        cnt, s, q = net.batchnorm_stats(n)
        assert cnt == 510
        assert np.linalg.norm(s - want[n][0]) <= 1e-6 * np.linalg.norm(want[n][0]), n
        assert np.linalg.norm(q - want[n][1]) <= 1e-6 * np.linalg.norm(want[n][1]), n
        mu = s / cnt
        pooled[n] = (mu, np.maximum(q / cnt - mu * mu, 0.0))
    assert net.batchnorm_commit() == 4
    net.set_batchnorm_train(False)
    net.forward(ba.ptr, 300)
    b2 = dict(bns)
    for n in TDNNF:
        m, v = pooled[n]
        b2[(n, 0)] = (m.astype(np.float32), v.astype(np.float32), np.ones(m.size, np.float32), np.zeros(m.size, np.float32))
    tp = {k: synth.trunc_fp16(v) for k, v in params.items()}
    on = oracle.OracleNet(xcfg, tp, b2, round_mode=oracle.ROUND_FUSED, threads=16)
    on.forward(fa.astype(np.float32))
    for name in TDNNF + ["prefinal-l", "prefinal-chain", "output"]:
        got, ref = net.read_activation(name).astype(np.float32), on.act(name)
        assert rel_fro(got, ref) <= 2e-3, (name, rel_fro(got, ref))
        assert max_abs_rel(got, ref) <= 1e-2, (name, max_abs_rel(got, ref))
    on.close()
    # the frozen forward does not accumulate; zero_stats clears; nothing left to commit
    assert net.batchnorm_stats("tdnnf5")[0] == 510
    net.batchnorm_zero_stats()
    for n in TDNNF:
        cnt, s, q = net.batchnorm_stats(n)
        assert cnt == 0 and not s.any() and not q.any()
    assert net.batchnorm_commit() == 0
    net.close()


def test_refusals(gpu):
    """MXFP8, implicit dz, row subsampling and nnet_backward_n with the mode: an error naming the
    other switch, in either order"""
    kf = gpu
    # (tdnnf8 at time-stride 3, so that the net admits row subsampling at all)
    xcfg = _xcfg().replace("name=tdnnf8 dim=256 bottleneck-dim=64 time-stride=1", "name=tdnnf8 dim=256 bottleneck-dim=64 time-stride=3")
    assert "time-stride=1" not in xcfg
    net, _, _ = _net(kf, xcfg)
    fb, gb = kf.upload_fp16(_features()), kf.upload_fp16(_out_grad())
    net.set_batchnorm_train(True)
    net.forward(fb.ptr, T)
    for call in (lambda: net.set_fp8(True), lambda: net.set_implicit_dz(True), lambda: net.set_row_subsampling(3),
                 lambda: kf.check(kf.nnet.nnet_backward_n(net.h, gb.ptr, 2), "nnet_backward_n")):
        with pytest.raises(kf.KfError, match="nnet_set_bn_train"):
            call()
    net.backward(gb.ptr)                  # the net still works
    net.set_batchnorm_train(False)
    net.forward(fb.ptr, T)
    kf.check(kf.nnet.nnet_backward_n(net.h, gb.ptr, 2), "nnet_backward_n")
    for on, off, name in ((lambda: net.set_fp8(True), lambda: net.set_fp8(False), "nnet_set_fp8"),
                          (lambda: net.set_implicit_dz(True), lambda: net.set_implicit_dz(False), "nnet_set_implicit_dz"),
                          (lambda: net.set_row_subsampling(3), lambda: net.set_row_subsampling(0), "nnet_set_row_subsampling")):
        on()
        with pytest.raises(kf.KfError, match=name):
            net.set_batchnorm_train(True)
        off()
    net.set_batchnorm_train(True)
    _run(net, fb, gb)
    kf.sync()
    net.close()


def test_refusal_data_parallel(gpu):
    """a net bound to data parallel refuses the mode, and a net in the mode refuses to be bound
    (nearly all of this test's time is the creation of the one-rank communicator)"""
    kf = gpu
    from kfp16 import dp
    net, _, _ = _net(kf, _xcfg())
    comm = dp.Communicator(0, 1, dp.unique_id(), 0)
    net.bind_dp(comm, 1 << 20)
    with pytest.raises(kf.KfError, match="nnet_bind_dp"):
        net.set_batchnorm_train(True)
    net.bind_dp(None, 0)
    net.set_batchnorm_train(True)
    with pytest.raises(kf.KfError, match="nnet_set_bn_train"):
        net.bind_dp(comm, 1 << 20)
    comm.close()
    net.close()


def test_trainer_composition(gpu, tmp_path):
    """EgsTrainer, three steps with training-mode BatchNorm, the Kaldi update, natural gradient, the
    orthonormal constraint at every step and a dropout schedule together"""
    kf = gpu
    import egs_writer as W
    from kfp16 import egs, synth, trainer
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, 4, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=4).next_batch()
    den = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)
    assert trainer.TrainConfig().batchnorm_train is False
    cfg = trainer.TrainConfig(learning_rate=1e-3, momentum=0.9, kaldi_update=True, max_param_change=1.0,
                              natural_gradient=True, orthonormal_every=1, dropout_schedule="0,0.3", dropout_seed=11,
                              total_steps=4, batchnorm_train=True)
    tr = trainer.EgsTrainer(_xcfg(dropout=True), den, max_egs=8, max_frames=800, config=cfg)
    synth.init_network(tr.net)
    for step in range(3):
        tr.step(batch, fraction=(step + 1) / 4)
        r = tr.result()
        assert r.num_ok == batch.batch_size and np.isfinite(r.objf)
        stats = tr.net.natural_gradient_stats()
        assert stats and not any(s["flag"] for s in stats)
        for n in TDNNF:
            assert tr.net.batchnorm_stats(n)[0] == (step + 1) * batch.total_frames
    assert tr.net.dropout_mask("tdnnf6").shape == (batch.batch_size, 256)
    assert tr.commit_batchnorm() == 4
