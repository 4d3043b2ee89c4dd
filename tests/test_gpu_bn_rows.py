"""Training-mode BatchNorm on the row-subsampled step (kf_ops.h kf_bn_train_bwd_*_rows, kf_nnet.h
nnet_set_bn_train_rows, TrainConfig.row_subsampling).

Kernels: the two _rows entries against float64 (tests/bn_rows_ref.py), bounds those of
test_gpu_bn_train.py's backward kernel test. Network: configs/tiny.xconfig with tdnnf8 at
time-stride 3 (tdnnf5 .. output then form the row set above cnn4), 3 sequences, the output gradient
on the rows 0 (mod 3) only, at 300 frames (T - 1 = 2 mod 3: a tail) and 298 (none), against the
staged reference on full rows (BnRowsOracle: statistics over the rows 0 (mod 3)). Bounds are
DESIGN §23's: 2e-3 relative Frobenius on activations and batch statistics, 5e-3 on gradients.

The rows of the set that are compared, and whose ReLU decisions are replayed: the rows c < tc0
(source rows 3c, exact at every layer) and the tail rows from tc0 + 4 on. The scratch slot tc0 is
not a row of the layer, and what it computes reaches one tail row further per 3-strided layer
above (three in this network: tc0 .. tc0 + 2 at the top); the margin is nnet_set_row_subsampling's
own. Elsewhere the reference keeps its own decisions."""
import os

import numpy as np
import pytest

import bn_rows_ref as rr
import bn_sites_ref as bs
import bn_train_ref as br
from conftest import rel_fro
from history_dev import tiny3_xcfg as _xcfg

pytestmark = pytest.mark.gpu

EPS = 1e-3
U24, U23 = 2.0 ** -24, 2.0 ** -23
TDNNF = ["tdnnf5", "tdnnf6", "tdnnf7", "tdnnf8"]
TOP = TDNNF + ["prefinal-l", "prefinal-chain", "output"]
EXACT_TAIL = 4          # tail rows tc0 + 4 .. are exact at every layer of tiny (see above)
ACT_TOL, GRAD_TOL = 2e-3, 5e-3


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------
# (rows, stat_rows): one row; a group of four straddling the threshold; the threshold on and just
# below the 256-row chunk boundary; four chunks with the threshold on a boundary, and at 1
ROWS = [(1, 1), (8, 5), (257, 256), (257, 250), (1031, 1024), (1031, 1)]
SHAPES = [(rows, srows, D, D) for rows, srows in ROWS for D in (8, 160, 1536)] + [(257, 250, 160, 192)]


def _r_matrix(rng, rows, D):
    """test_gpu_bn_train.py's: column 0 all zero, 1 constant, 2 mean 4 with deviation 1/64"""
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


class _Bwd:
    """the inputs of one backward kernel case on the device"""

    def __init__(self, kf, rows, srows, D, ld, with_drop, with_mask, seed):
        rng = np.random.default_rng(seed)
        self.kf, self.rows, self.srows, self.D, self.ld, self.rms = kf, rows, srows, D, ld, 0.75
        self.r16 = _r_matrix(rng, rows, D)
        self.g16 = (rng.standard_normal((rows, D)) * 0.1).astype(np.float16)
        fwd = br.bn_train_forward(self.r16[:srows].astype(np.float64), EPS, self.rms)
        self.sc32, self.sh32 = fwd["scale"].astype(np.float32), fwd["shift"].astype(np.float32)
        self.seg = (np.arange(rows) * 3) // rows
        self.drop = rng.uniform(0.4, 1.6, size=(3, D)).astype(np.float32) if with_drop else None
        self.bits = rng.integers(0, 2, size=(rows, D)).astype(np.uint8) if with_mask else np.ones((rows, D), np.uint8)
        packed = np.packbits(self.bits.reshape(-1), bitorder="little")
        self.gb, self.rb = kf.upload_fp16(_pad(self.g16, ld, 5)), kf.upload_fp16(_pad(self.r16, ld, 7))
        self.scb, self.shb = kf.upload_f32(self.sc32), kf.upload_f32(self.sh32)
        self.ab = kf.upload_f32(np.zeros(2 * D, np.float32))
        self.db = kf.upload_f32(self.drop) if with_drop else None
        self.sb = kf.upload_f32(self.seg.astype(np.int32).view(np.float32)) if with_drop else None
        self.mb = kf.upload_f32(np.frombuffer(packed.tobytes() + b"\0" * (-len(packed) % 4), np.float32)) if with_mask else None
        self.dzb = kf.upload_fp16(np.full((rows, ld), 9, np.float16))

    def run(self, entry="rows"):
        kf, D, ld, rows = self.kf, self.D, self.ld, self.rows
        dp, sp = (self.db.ptr, self.sb.ptr) if self.db else (None, None)
        mp = self.mb.ptr if self.mb else None
        a, b = self.ab.ptr, self.ab.ptr + 4 * D
        if entry == "rows":
            kf.check(kf.core.kf_bn_train_bwd_stats_rows(self.gb.ptr, ld, self.rb.ptr, ld, rows, self.srows, D, self.scb.ptr,
                                                        self.shb.ptr, self.rms, dp, D, sp, a, b), "kf_bn_train_bwd_stats_rows")
            kf.check(kf.core.kf_bn_train_bwd_apply_rows(self.gb.ptr, ld, self.rb.ptr, ld, rows, self.srows, D, self.scb.ptr,
                                                        self.shb.ptr, self.rms, a, b, dp, D, sp, mp, D, self.dzb.ptr, ld),
                     "kf_bn_train_bwd_apply_rows")
        else:
            kf.check(kf.core.kf_bn_train_bwd_stats(self.gb.ptr, ld, self.rb.ptr, ld, rows, D, self.scb.ptr, self.shb.ptr,
                                                   self.rms, dp, D, sp, a, b), "kf_bn_train_bwd_stats")
            kf.check(kf.core.kf_bn_train_bwd_apply(self.gb.ptr, ld, self.rb.ptr, ld, rows, D, self.scb.ptr, self.shb.ptr,
                                                   self.rms, a, b, dp, D, sp, mp, D, self.dzb.ptr, ld), "kf_bn_train_bwd_apply")
        return kf.read_f32(self.ab.ptr, (2, D)), kf.read_fp16(self.dzb.ptr, (rows, ld))


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("with_drop", [False, True])
@pytest.mark.parametrize("rows,srows,D,ld", SHAPES)
def test_rows_kernels_against_float64(gpu, rows, srows, D, ld, with_drop, with_mask):
    c = _Bwd(gpu, rows, srows, D, ld, with_drop, with_mask, rows * 11 + srows + D + with_drop + 2 * with_mask)
    r, g = c.r16.astype(np.float64), c.g16.astype(np.float64)
    sc, sh, rms = c.sc32.astype(np.float64), c.sh32.astype(np.float64), c.rms
    S = np.arange(srows)
    a_ref, b_ref, gr = rr.bn_rows_backward(g, r, S, sc, sh, rms, c.drop, c.seg if with_drop else None)
    dz_ref = gr * c.bits
    ab1, dz1 = c.run()
    a, b = ab1[0].astype(np.float64), ab1[1].astype(np.float64)
    dy = g * (c.drop[c.seg].astype(np.float64) if with_drop else 1.0)
    # test_gpu_bn_train.py's bounds with the divisor n = stat_rows: fp32 storage of double sums, the
    # absolute term on the terms' magnitudes (b cancels where a column's mean is far above its deviation)
    ba = U23 * np.abs(a_ref) + 1e-12 * np.abs(dy).sum(0) / srows
    bb = U23 * np.abs(b_ref) + 1e-12 * (np.abs(sc) * np.abs(dy * r).sum(0) + np.abs(sh) * np.abs(dy).sum(0)) / (rms * srows)
    assert np.all(np.abs(a - a_ref) <= ba)
    assert np.all(np.abs(b - b_ref) <= bb)
    yhat = (r * sc + sh) / rms
    tol = _f16_ulp(dz_ref) + np.abs(sc) * (ba + np.abs(yhat) * bb)
    got = dz1[:, :D].astype(np.float64)
    err = np.abs(got - dz_ref)
    print("dz err / tol max %.3g" % np.max(err / tol))
    assert np.all(err[:srows] <= tol[:srows])
    # the rows from stat_rows on, on their own: rne(scale dy relu_bit) and nothing of a or b. scale dy
    # is exact in double, so the only error is the store's rounding (one fp16 ulp covers a float step
    # between); a correction applied there would be off by scale |a + yhat b|, far more wherever a != 0
    tail_ref = sc * dy[srows:] * c.bits[srows:]
    assert np.all(np.abs(got[srows:] - tail_ref) <= _f16_ulp(tail_ref))
    if rows > srows:
        wrong = np.abs(gr[srows:] - (sc * (dy - a_ref - yhat * b_ref))[srows:]) * c.bits[srows:]
        assert np.any(wrong > 4 * _f16_ulp(tail_ref)), "the case cannot tell a correction on the tail rows"
    assert np.all(dz1[:, :D][c.bits == 0] == 0)
    assert np.all(dz1[:, D:] == 9)                        # nothing past D is written
    ab2, dz2 = c.run()
    assert np.array_equal(ab1.view(np.uint32), ab2.view(np.uint32)) and np.array_equal(dz1.view(np.uint16), dz2.view(np.uint16))


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("with_drop", [False, True])
@pytest.mark.parametrize("rows,D,ld", [(1, 8, 8), (8, 160, 160), (257, 160, 192), (1031, 1536, 1536)])
def test_rows_kernels_equal_the_existing_entries(gpu, rows, D, ld, with_drop, with_mask):
    """stat_rows == rows: kf_bn_train_bwd_stats / _apply bit for bit"""
    c = _Bwd(gpu, rows, rows, D, ld, with_drop, with_mask, rows + D)
    ab1, dz1 = c.run("rows")
    ab0, dz0 = c.run("old")
    assert np.array_equal(ab1.view(np.uint32), ab0.view(np.uint32))
    assert np.array_equal(dz1.view(np.uint16), dz0.view(np.uint16))


def test_rows_kernel_argument_checks(gpu):
    kf = gpu
    buf = kf.upload_f32(np.zeros(256, np.float32))
    p = buf.ptr
    for srows in (0, 5, -1):
        assert kf.core.kf_bn_train_bwd_stats_rows(p, 8, p, 8, 4, srows, 8, p, p, 1.0, None, 0, None, p, p) == -1
        assert b"kf_bn_train_bwd_stats_rows" in kf.core.kf_last_error()
        assert kf.core.kf_bn_train_bwd_apply_rows(p, 8, p, 8, 4, srows, 8, p, p, 1.0, p, p, None, 0, None, None, 0, p + 512, 8) == -1
        assert b"kf_bn_train_bwd_apply_rows" in kf.core.kf_last_error()
    assert kf.core.kf_bn_train_bwd_stats_rows(p, 12, p, 12, 4, 2, 12, p, p, 1.0, None, 0, None, p, p) == -1   # D % 8
    assert kf.core.kf_bn_train_bwd_stats_rows(p, 8, p, 8, 4, 4, 8, p, p, 1.0, None, 0, None, p, p + 64) == 0
    kf.sync()


# ---------------------------------------------------------------------------
# network
# ---------------------------------------------------------------------------
def _seq(frames):
    return np.asarray([0, 90, 200, frames], np.int32)


def _features(frames, seed=1234):
    from kfp16 import synth
    return synth.make_features(frames, 40, seed=seed)


def _out_grad(frames, seed=7):
    """on the rows 0 (mod 3) only: what row subsampling declares"""
    og = np.zeros((frames, 200), np.float16)
    og[::3] = (np.random.default_rng(seed).standard_normal((len(og[::3]), 200)) * 0.05).astype(np.float16)
    return og


def _net(kf, xcfg, frames, sites="tdnnf", bns=None, policy="subsampled", rsub=True, train=True):
    from kfp16 import synth
    net = kf.Network(xcfg, max_frames=300)
    params, bns0 = synth.init_network(net)
    if bns is not None:
        for (name, which), (m, v, g, b) in bns.items():
            net.set_bn(name, which, m, v, g, b, eps=1e-3)
    net.set_sequences(_seq(frames))
    if policy is not None:
        net.set_batchnorm_train_rows(policy)
    if rsub:
        net.set_row_subsampling(3)
    if sites != "tdnnf":
        net.set_batchnorm_train_sites(sites)
    if train:
        net.set_batchnorm_train(True)
    return net, params, bns0 if bns is None else bns


def _step(kf, net, frames, og=None):
    """one forward / backward; the output gradient goes in the forward's row form.
    -> (output, gradients, (tc, tc0, rows))"""
    fb = kf.upload_fp16(_features(frames))
    net.forward(fb.ptr, frames)
    tc, tc0, rows = net.row_set()
    og = _out_grad(frames) if og is None else og
    gb = kf.upload_fp16(og[rows] if tc else og)
    out = net.read_activation("output").copy()
    net.backward(gb.ptr)
    return out, net.read_grads(), (tc, tc0, rows)


def _governed(net):
    out = []
    for n in net.batchnorm_train_layers():
        out.append((n, 0))
        if n.startswith("prefinal"):
            out.append((n, 1))
    return out


def _stat_errors(key, got, want):
    """test_gpu_bn_sites.py's: relative Frobenius, but a prefinal layer's BatchNorm 1 sees a tensor
    whose column mean is rounding noise around 0 (BatchNorm 0 made it so); its mean is held per
    column to 2e-3 of the column's rms"""
    (m, v), (mr, vr) = got, want
    em, ev = rel_fro(m, mr), rel_fro(v, vr)
    if key[1] == 1:
        em = float(np.max(np.abs(m - mr) / np.sqrt(vr + mr * mr)))
    return em, ev


def _compare(kf, frames, sites, dropout):
    """the GPU's row-subsampled train-mode step against the staged full-row reference"""
    import oracle  # noqa: F401  (the staged oracles import it)
    from kfp16 import synth
    xcfg = _xcfg(dropout)
    feats, og = _features(frames), _out_grad(frames)
    site_list = sites.split(",")
    bns = None
    if "prefinal" in site_list:
        # (the frozen layers below a governed prefinal-layer carry statistics that match the data,
        # bn_sites_ref.matched_bns: under random ones the comparison from the features is ill-conditioned)
        probe = kf.Network(xcfg, max_frames=300)
        params, bns0 = synth.init_network(probe)
        probe.close()
        tp = {k: synth.trunc_fp16(v) for k, v in params.items()}
        bns = bs.matched_bns(xcfg, tp, bns0, feats.astype(np.float32), site_list, threads=16)
    net, params, bns = _net(kf, xcfg, frames, sites, bns)
    if dropout:
        net.set_dropout_proportion(0.3)
        net.set_dropout(True, 0x5EED5EED12345678)
    fb = kf.upload_fp16(feats)
    net.forward(fb.ptr, frames)
    tc, tc0, rows = net.row_set()
    assert tc0 == (frames - 1) // 3 + 1 and (tc > tc0) == ((frames - 1) % 3 != 0), (tc, tc0)
    exact = np.concatenate([np.arange(tc0), np.arange(tc0 + EXACT_TAIL, tc)]).astype(np.int64)
    gov = _governed(net)
    acts = {n: net.read_activation(n).astype(np.float32) for n in TOP}
    assert all(a.shape[0] == tc for a in acts.values())
    # (tiny's cnn4 subsamples the height, so it is not evaluated on the compact rows: its mask is in full rows)
    on_set = TDNNF + ["prefinal-chain"] + (["cnn4"] if net.read_activation("cnn4").shape[0] == tc else [])
    stats = {k: net.batchnorm_batch_stats(*k) for k in gov}
    masks = {n: net.dropout_mask(n) for n in TDNNF} if dropout else None
    relu = net.relu_masks()
    gb = kf.upload_fp16(og[rows])
    net.backward(gb.ptr)
    grads = net.read_grads()
    net.close()

    tp = {k: synth.trunc_fp16(v) for k, v in params.items()}
    if dropout:
        inner = br.BnTrainOracle(xcfg, tp, bns, TDNNF, masks=masks, seq_row0=_seq(frames), threads=16)
    else:
        inner = bs.BnSitesOracle(xcfg, tp, bns, site_list, threads=16)
    ref = rr.BnRowsOracle(inner)
    ref.forward(feats.astype(np.float32))
    S = rr.rows_mod3(frames)
    worst = 0.0
    for n in TOP:
        e = rel_fro(acts[n][exact], ref.act(n)[rows[exact]])
        worst = max(worst, e / ACT_TOL)
        assert e <= ACT_TOL, (n, e)
    sep = {}
    for k in gov:
        want = ref.stats_of(*k)
        em, ev = _stat_errors(k, stats[k], want)
        worst = max(worst, em / ACT_TOL, ev / ACT_TOL)
        assert em <= ACT_TOL and ev <= ACT_TOL, (k, em, ev)
        # the rule against the parent's: the statistics of the same r over every row lie far away
        r = ref.r_of(*k)
        assert np.abs(r[S].mean(0) - want[0]).max() <= 1e-9
        allrows = (r.mean(0), r.var(0))
        sep[k] = _stat_errors(k, stats[k], allrows)
    # ReLU decisions: the reference's own, the GPU's on the compared rows of the set
    own = ref.relu_decisions()
    force = {}
    for n, m in own.items():
        w = m.size // frames
        if n in on_set:                                 # the row set (and a conv evaluated on it)
            mm = m.reshape(frames, w).copy()
            mm[rows[exact]] = relu[n][:tc * w].reshape(tc, w)[exact]
            force[n] = mm.reshape(-1)
        else:
            force[n] = relu[n]
    ref.forward(feats.astype(np.float32), force_masks=force)
    want = ref.backward(og.astype(np.float32))
    ref.close()
    errs = {k: rel_fro(grads[k], want[k]) for k in want}
    print("worst forward error / tolerance %.2f; separation %s; grad errors: %s" % (
        worst, ", ".join("%s/%d=%.1e,%.1e" % (k[0], k[1], a, b) for k, (a, b) in sep.items()),
        ", ".join(f"{k}={v:.2e}" for k, v in errs.items())))
    assert set(errs) == set(grads)
    bad = {k: v for k, v in errs.items() if v > GRAD_TOL}
    assert not bad, bad
    return sep


@pytest.mark.parametrize("frames", [300, 298])
def test_network_against_reference(gpu, frames):
    sep = _compare(gpu, frames, "tdnnf", False)
    # the separation: the GPU's batch statistics are not the all-rows statistics of the same r
    for k, (em, ev) in sep.items():
        assert em > 5 * ACT_TOL and ev > 5 * ACT_TOL, (k, em, ev)


def test_network_with_dropout(gpu):
    _compare(gpu, 300, "tdnnf", True)


def test_network_tdnnf_and_prefinal(gpu):
    sep = _compare(gpu, 300, "tdnnf,prefinal", False)
    for k, (em, ev) in sep.items():
        assert em > 5 * ACT_TOL and ev > 5 * ACT_TOL, (k, em, ev)


# ---------------------------------------------------------------------------
# invariants
# ---------------------------------------------------------------------------
def test_counts_and_column_means(gpu):
    """count grows by tc0 per compact forward and by T per full-row forward; the BatchNorm part of
    a governed layer has column mean 0 over the rows of S (test_network_forward's 2^-10)"""
    kf = gpu
    net, _, _ = _net(kf, _xcfg(), 300, "tdnnf,prefinal")
    net.batchnorm_zero_stats()
    fb = kf.upload_fp16(_features(300))
    net.forward(fb.ptr, 300)
    tc, tc0, _ = net.row_set()
    assert tc0 == 100 and tc > tc0
    acts = {n: net.read_activation(n).astype(np.float64) for n in TDNNF}
    for name, below in (("tdnnf6", "tdnnf5"), ("tdnnf7", "tdnnf6"), ("tdnnf8", "tdnnf7")):
        y = acts[name][:tc0] - 0.66 * acts[below][:tc0]
        print("%s: max |column mean over S| %.2e" % (name, np.abs(y.mean(0)).max()))
        assert np.abs(y.mean(0)).max() <= 2.0 ** -10
    for k in _governed(net):
        assert net.batchnorm_stats(*k)[0] == tc0, k
    net.forward(fb.ptr, 298)                      # no tail
    assert net.row_set()[:2] == (100, 100)
    net.set_row_subsampling(0)                    # full rows
    net.forward(fb.ptr, 300)
    assert net.row_set()[0] == 0
    for k in _governed(net):
        assert net.batchnorm_stats(*k)[0] == 2 * tc0 + 300, k
    net.set_row_subsampling(3)
    net.forward(fb.ptr, 101)                      # too short for a row set with a tail: full rows again
    assert net.row_set()[0] == 0
    for k in _governed(net):
        assert net.batchnorm_stats(*k)[0] == 2 * tc0 + 401, k
    net.close()


def test_step_replays_and_policy_alone_changes_nothing(gpu):
    kf = gpu
    net, _, _ = _net(kf, _xcfg(), 300)
    o1, g1, rs = _step(kf, net, 300)
    assert rs[0] > rs[1] > 0
    net.set_wgrad_stream(False)
    o2, g2, _ = _step(kf, net, 300)
    net.set_wgrad_stream(True)
    o3, g3, _ = _step(kf, net, 300)
    for o, g in ((o2, g2), (o3, g3)):
        assert np.array_equal(o.view(np.uint16), o1.view(np.uint16))
        for k in g1:
            assert np.array_equal(g[k].view(np.uint32), g1[k].view(np.uint32)), k
    # the setter while both modes are on
    assert net.batchnorm_train_rows() == "subsampled"
    with pytest.raises(kf.KfError, match="set_bn_train_rows"):
        net.set_batchnorm_train_rows("all")
    net.set_batchnorm_train_rows("subsampled")    # (no change: not refused)
    with pytest.raises(kf.KfError):
        net.set_batchnorm_train_rows("some")
    assert kf.nnet.nnet_set_bn_train_rows(net.h, 2) == -1
    net.set_batchnorm_train(False)
    net.set_batchnorm_train_rows("all")
    # the default policy: the two modes refuse each other, in either order, as they always did
    with pytest.raises(kf.KfError, match="not supported with row subsampling \\(nnet_set_row_subsampling\\)"):
        net.set_batchnorm_train(True)
    net.set_row_subsampling(0)
    net.set_batchnorm_train(True)
    with pytest.raises(kf.KfError, match="not supported with training-mode BatchNorm on \\(nnet_set_bn_train\\)"):
        net.set_row_subsampling(3)
    net.close()
    # the policy with the mode off: the row-subsampled step of a net that never set it, bit for bit
    outs = []
    for policy in (None, "subsampled"):
        net, _, _ = _net(kf, _xcfg(), 300, policy=policy, train=False)
        outs.append(_step(kf, net, 300))
        net.close()
    assert outs[0][2][0] == outs[1][2][0] > 0
    assert np.array_equal(outs[0][0].view(np.uint16), outs[1][0].view(np.uint16))
    for k, v in outs[0][1].items():
        assert np.array_equal(v.view(np.uint32), outs[1][1][k].view(np.uint32)), k


@pytest.mark.parametrize("sites", ["all", "tdnnf"])
def test_sites_on_the_benchmark_model(gpu, sites):
    """T = 3000. KF_BN_SITE_ALL: the governed conv below the row set (cnn6) runs on full rows through
    the gather path, so the step is that of KF_RSUB_CONV=0 bit for bit, and cnn6's statistics run
    over all T x height-out block rows. The tdnnf sites: cnn6 is frozen and evaluated on the compact
    rows, which gives what the gather path gives (test_gpu_row_subsampling.py: cnn6's rows bit for
    bit, the gradients at 1e-5, another split-K order)"""
    kf = gpu
    from kfp16 import synth
    xcfg = synth.load_xconfig("cnn_tdnn_17f.xconfig")
    T = 3000
    feats = synth.make_features(T, 40)
    og = np.zeros((T, 0), np.float16)
    res = []
    for conv_env in (None, "0"):
        net = kf.Network(xcfg, max_frames=T)
        synth.init_network(net, seed=42)
        net.set_batchnorm_train_rows("subsampled")
        if conv_env is not None:
            os.environ["KF_RSUB_CONV"] = conv_env
        try:
            net.set_row_subsampling(3)
        finally:
            os.environ.pop("KF_RSUB_CONV", None)
        net.set_batchnorm_train_sites(sites)
        net.set_batchnorm_train(True)
        net.batchnorm_zero_stats()
        fb = kf.upload_fp16(feats)
        net.forward(fb.ptr, T)
        tc, tc0, rows = net.row_set()
        assert tc > tc0 == 1000
        P = net.layers[-1][3]
        if og.shape[1] != P:
            og = np.zeros((T, P), np.float16)
            sup = np.concatenate([np.arange(1500 * e + 30, 1500 * (e + 1), 3) for e in range(2)])
            og[sup] = (np.random.default_rng(3).standard_normal((len(sup), P)) * 0.05).astype(np.float16)
        gb = kf.upload_fp16(og[rows])
        out = net.read_activation("output").copy()
        cnn6 = net.read_activation("cnn6")
        net.backward(gb.ptr)
        grads = net.read_grads()
        assert net.batchnorm_stats("tdnnf7")[0] == tc0 and net.batchnorm_stats("tdnnf23")[0] == tc0
        if sites == "all":
            assert cnn6.shape[0] == T             # full rows, whatever KF_RSUB_CONV says
            dims = {n: dout for n, _ty, _din, dout in net.layers}
            hout = dims["cnn6"] // net._bn_dim("cnn6")
            assert net.batchnorm_stats("cnn6")[0] == T * hout
            assert net.batchnorm_stats("prefinal-chain", 1)[0] == tc0
        else:
            assert cnn6.shape[0] == (T if conv_env == "0" else tc)
            cnn6 = cnn6[:tc] if conv_env != "0" else cnn6[rows]
        assert all(np.all(np.isfinite(v)) for v in grads.values())
        res.append((out, cnn6, grads))
        net.close()
    assert np.array_equal(res[0][0][:1000].view(np.uint16), res[1][0][:1000].view(np.uint16))
    assert np.array_equal(res[0][1].view(np.uint16), res[1][1].view(np.uint16))
    for k, v in res[0][2].items():
        assert np.any(v), k
        if sites == "all":
            assert np.array_equal(res[0][0].view(np.uint16), res[1][0].view(np.uint16))
            assert np.array_equal(v.view(np.uint32), res[1][2][k].view(np.uint32)), k
        else:
            assert rel_fro(v, res[1][2][k]) <= 1e-5, (k, rel_fro(v, res[1][2][k]))


# ---------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------
def _egs(tmp_path, n=4):
    import egs_writer as W
    from kfp16 import egs, synth
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, n, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=n).next_batch()
    return batch, synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)


def test_trainer_row_subsampling_matches_full_rows(gpu, tmp_path):
    """frozen BatchNorm: the row-subsampled trainer step reads the same supervised rows (objf bit-equal)
    and leaves the full-row step's gradients (test_gpu_row_subsampling.py's 1e-5: another split-K order)"""
    from kfp16 import synth, trainer
    batch, den = _egs(tmp_path)
    row0, _ = trainer.chain_rows(batch.frame_offsets, batch.num_frames, batch.frames_per_seq, 3, 30)
    assert np.all(row0 % 3 == 0)
    assert trainer.TrainConfig().row_subsampling is False and trainer.TrainConfig().batchnorm_train_rows == "all"
    res = []
    for rsub in (False, True):
        cfg = trainer.TrainConfig(learning_rate=0.0, momentum=0.0, row_subsampling=rsub)
        tr = trainer.EgsTrainer(_xcfg(), den, max_egs=8, max_frames=800, config=cfg)
        synth.init_network(tr.net)
        tr.step(batch)
        r = tr.result()
        assert r.num_ok == batch.batch_size and np.isfinite(r.objf)
        assert (tr.net.row_set()[0] > 0) == rsub and tr.full_row_steps == 0
        res.append((r.objf, tr.net.read_grads()))
        tr.net.close()
    assert res[0][0] == res[1][0]
    for k, v in res[0][1].items():
        assert np.any(v), k
        assert rel_fro(res[1][1][k], v) <= 1e-5, (k, rel_fro(res[1][1][k], v))


def test_trainer_composition(gpu, tmp_path):
    """three steps with row subsampling, training-mode BatchNorm on the subsampled rows, the Kaldi
    update, NG-SGD, the orthonormal constraint, a dropout schedule and xent_regularize together"""
    kf = gpu
    from kfp16 import synth, trainer
    batch, den = _egs(tmp_path)
    xcfg = synth.load_xconfig("tiny_xent.xconfig")
    assert xcfg.count("bypass-scale=0.66") == 2
    xcfg = xcfg.replace("bypass-scale=0.66", "bypass-scale=0.66 dropout-proportion=0.0")
    kw = dict(learning_rate=1e-3, momentum=0.9, kaldi_update=True, max_param_change=1.0, natural_gradient=True,
              orthonormal_every=1, dropout_schedule="0,0.3", dropout_seed=11, total_steps=4, batchnorm_train=True,
              batchnorm_train_sites="tdnnf,prefinal", xent_regularize=0.1, row_subsampling=True)
    # without the policy the constructor raises the library's refusal
    with pytest.raises(kf.KfError, match="not supported with row subsampling"):
        trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=800, config=trainer.TrainConfig(**kw))
    tr = trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=800,
                            config=trainer.TrainConfig(batchnorm_train_rows="subsampled", **kw))
    synth.init_network(tr.net)
    assert tr.net.batchnorm_train_rows() == "subsampled"
    T = batch.total_frames
    tc0 = (T - 1) // 3 + 1
    for step in range(3):
        tr.step(batch, fraction=(step + 1) / 4)
        r = tr.result()
        assert r.num_ok == batch.batch_size and np.isfinite(r.objf) and np.isfinite(r.xent_objf)
        tc, got_tc0, _ = tr.net.row_set()
        assert tc >= got_tc0 == tc0
        stats = tr.net.natural_gradient_stats()
        assert stats and not any(s["flag"] for s in stats)
        for k in _governed(tr.net):
            assert tr.net.batchnorm_stats(*k)[0] == (step + 1) * tc0, k
    assert tr.full_row_steps == 0
    assert all(np.all(np.isfinite(v)) for v in tr.net.get_params().values())
    assert tr.commit_batchnorm() == 4
    tr.net.close()


def test_trainer_unaligned_batch_takes_the_full_row_step(gpu, tmp_path):
    from kfp16 import synth, trainer
    batch, den = _egs(tmp_path)
    cfg = trainer.TrainConfig(learning_rate=1e-3, momentum=0.0, row_subsampling=True)
    tr = trainer.EgsTrainer(_xcfg(), den, max_egs=8, max_frames=800, config=cfg)
    synth.init_network(tr.net)
    tr.step(batch)
    assert np.isfinite(tr.result().objf) and tr.full_row_steps == 0 and tr.net.row_set()[0] > 0
    off = np.array(batch.frame_offsets, np.int32)
    off[1] += 1                                   # that eg's first supervised row is 1 (mod 3) now
    batch.frame_offsets = off
    tr.step(batch)
    r = tr.result()
    assert r.num_ok == batch.batch_size and np.isfinite(r.objf)
    assert tr.full_row_steps == 1 and tr.net.row_set()[0] == 0
    batch.frame_offsets = off - np.array([0, 1, 0, 0], np.int32)
    tr.step(batch)                                # and the next aligned batch is row-subsampled again
    assert np.isfinite(tr.result().objf) and tr.full_row_steps == 1 and tr.net.row_set()[0] > 0
    tr.net.close()
