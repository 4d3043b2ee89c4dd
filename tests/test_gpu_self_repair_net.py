"""ReLU unit statistics and self-repair through the network and the trainer (kf_nnet.h
nnet_set_self_repair, TrainConfig.self_repair) on configs/tiny.xconfig: 300 frames,
3 sequences, training-mode BatchNorm on every site.

Dead and saturated units are made after synth.init_network: a bias of -30 / +30 on a few columns of
tdnnf6's affine and of prefinal-chain's big affine and on a few filters of cnn2.
test_setup_is_dead_and_saturated holds that deriv_avg is exactly 0 and 1 there.

What is compared with what:
- statistics: exact, against the column popcount of the network's own ReLU masks;
- a dead unit's bias gradient: its ReLU bit is 0 on every row, so dz is rne_fp16(s) there and the
  gradient -rne_fp16(k) n (n H for a conv filter), to DESIGN §23's 5e-3 on gradients;
- the strided layers: with a zero output gradient and every other site at scale 0 the layer's own
  gradients are the response to dz = 1 (x) s alone, restated in numpy with the clamped splices'
  edge rows (self_repair_ref.tdnnf_response), 5e-3 relative Frobenius;
- the whole step at k = 2^-10, on all rows with every site governed and row-subsampled with the tdnnf
  and prefinal sites: activations and batch statistics (2e-3), the unit statistics (exact, with the
  GPU's ReLU decisions replayed) and every gradient (5e-3) against the staged reference
  (self_repair_ref.SelfRepairOracle, under bn_rows_ref.BnRowsOracle for the row-subsampled step).
"""
import numpy as np
import pytest

import self_repair_ref as sr
from conftest import rel_fro
from history_dev import tiny3_xcfg

pytestmark = pytest.mark.gpu

GRAD_TOL = 5e-3
FRAMES = 300
DEAD = {"tdnnf6": ("tdnnf6.AffineBias", [3, 77, 200]), "tdnnf7": ("tdnnf7.AffineBias", [10, 100]), "cnn2": ("cnn2.Bias", [5, 30]),
        "prefinal-chain": ("prefinal-chain.BigBias", [0, 129])}
SAT = {"tdnnf6": ("tdnnf6.AffineBias", [4, 78]), "tdnnf7": ("tdnnf7.AffineBias", [11]), "cnn2": ("cnn2.Bias", [6]),
       "prefinal-chain": ("prefinal-chain.BigBias", [1, 255])}
HEIGHT = {"cnn1": 40, "cnn2": 20, "cnn3": 20, "cnn4": 10}
K10 = 2.0 ** -10


def _seq(frames):
    return np.asarray([0, 90, 200, frames], np.int32)


def _features(frames, seed=1234):
    from kfp16 import synth
    return synth.make_features(frames, 40, seed=seed)


def _out_grad(frames, seed=7, mod3=False):
    og = (np.random.default_rng(seed).standard_normal((frames, 200)) * 0.05).astype(np.float16)
    if mod3:
        og[np.arange(frames) % 3 != 0] = 0
    return og


def _net(kf, xcfg=None, bn_train=True, self_repair=True, k=None, rsub=False, sites="all"):
    """a net with the dead and saturated units; k: every site's scale (None: the xconfig's)"""
    from kfp16 import synth
    net = kf.Network(xcfg or synth.load_xconfig("tiny.xconfig"), max_frames=FRAMES)
    params, _ = synth.init_network(net)
    for table, v in ((DEAD, -30.0), (SAT, 30.0)):
        for name, cols in table.values():
            params[name] = params[name].copy()
            params[name][0, cols] = v
    net.set_params(params)
    net.set_sequences(_seq(FRAMES))
    if rsub:
        net.set_batchnorm_train_rows("subsampled")
        net.set_row_subsampling(3)
    net.set_batchnorm_train_sites(sites)
    if bn_train:
        net.set_batchnorm_train(True)
    if self_repair:
        net.set_self_repair(True)
        if k is not None:
            for name in net.self_repair_sites():
                net.set_self_repair_opts(name, k)
    return net


def _step(kf, net, frames=FRAMES, og=None, backward=True):
    fb = kf.upload_fp16(_features(frames))
    net.forward(fb.ptr, frames)
    out = net.read_activation("output").copy()
    if not backward:
        return out, None
    tc, _tc0, rows = net.row_set()
    og = _out_grad(frames) if og is None else og
    gb = kf.upload_fp16(og[rows] if tc else og)
    net.backward(gb.ptr)
    return out, {k: v.copy() for k, v in net.read_grads().items()}


def _popcount(net, name, rows):
    """column popcount of the layer's ReLU mask over its first `rows` rows (a conv: per filter)"""
    m = net.relu_masks()[name]
    width = m.size // net.T
    F = width // HEIGHT.get(name, 1)
    return m.reshape(net.T, width)[:rows].reshape(-1, F).sum(0).astype(np.float64)


SITES = ["cnn1", "cnn2", "cnn3", "cnn4", "tdnnf5", "tdnnf6", "tdnnf7", "tdnnf8", "prefinal-chain"]


def test_setup_is_dead_and_saturated(gpu):
    net = _net(gpu)
    assert net.self_repair_sites() == SITES
    _step(gpu, net, backward=False)
    for table, want in ((DEAD, 0.0), (SAT, 1.0)):
        for layer, (_, cols) in table.items():
            st = net.relu_stats(layer)
            assert np.all(st["deriv_avg"][cols] == want), (layer, st["deriv_avg"][cols])
    net.close()


def test_statistics(gpu):
    kf = gpu
    net = _net(kf)
    want = {}
    for frames in (300, 210):
        if frames != FRAMES:
            net.set_sequences(np.asarray([0, 90, frames], np.int32))
        _step(kf, net, frames, backward=False)
        for name in SITES:
            want[name] = want.get(name, 0) + _popcount(net, name, frames)
    for name in SITES:
        cnt, vsum, dsum = net.relu_stats_raw(name)
        assert cnt == 510 * HEIGHT.get(name, 1), name
        # the mask bit is v > 0 before the fp16 rounding, the count reads r > 0 after it: they differ
        # only for 0 < v < 2^-25, which rounds to 0
        assert np.array_equal(dsum, want[name]), \
            f"{name}: deriv_sum differs from the masks' popcount (an element with 0 < v < 2^-25 rounds to r = 0?)"
        bcnt, bsum, _ = net.batchnorm_stats(name, 0)
        assert bcnt == cnt and np.array_equal(vsum, bsum)
        st = net.relu_stats(name)
        assert np.array_equal(st["value_avg"], bsum / bcnt) and np.array_equal(st["deriv_avg"], dsum / cnt)
    net.relu_zero_stats()
    for name in SITES:
        cnt, vsum, dsum = net.relu_stats_raw(name)
        assert cnt == 0 and not vsum.any() and not dsum.any()
        assert not net.relu_stats(name)["deriv_avg"].any()
    net.close()


@pytest.mark.parametrize("k", [K10, 1e-5], ids=["k=2^-10", "k=1e-5"])
def test_dead_unit_bias_gradient(gpu, k):
    """The test that fails without the feature: a dead unit's bias gradient is 0 there. At Kaldi's
    1e-5 (no loss scale) rne_fp16(k) is an fp16 subnormal, 168 x 2^-24: the gradient holds only if the
    subnormal dz survives the weight-gradient kernels' operand path."""
    kf = gpu
    net = _net(kf, k=k)
    p0 = net.get_params()
    _, g = _step(kf, net)
    k16 = float(np.float16(np.float32(k)))
    n = FRAMES
    for layer, (pname, cols) in DEAD.items():
        s = net.self_repair_vector(layer)
        assert np.all(s[cols] == -np.float32(k))
        want = -k16 * n * HEIGHT.get(layer, 1)
        got = g[pname][0, cols].astype(np.float64)
        print(f"{layer} dead bias gradient {got} want {want:.6g}")
        assert np.all(np.abs(got - want) <= GRAD_TOL * abs(want)), (layer, got, want)
    for layer, (pname, cols) in SAT.items():
        assert np.all(net.self_repair_vector(layer)[cols] == np.float32(k))
    net.sgd(0.5, 0.0)
    p1 = net.get_params()
    for layer, (pname, cols) in DEAD.items():
        assert np.all(p1[pname][0, cols] > p0[pname][0, cols]), layer
    net.close()


@pytest.mark.parametrize("layer,below", [("tdnnf6", "tdnnf5"), ("tdnnf7", "tdnnf6")])
def test_strided_layer_gradients_are_the_response_to_the_term(gpu, layer, below):
    """a zero output gradient and every other site at scale 0: the layer's dz is rne_fp16(s) on every
    row, masked-out elements included, and its linear weight gradient sums the stored rows into the
    clamped splice's edge row"""
    kf = gpu
    net = _net(kf, k=0.0)
    net.set_self_repair_opts(layer, K10)
    _, g = _step(kf, net, og=np.zeros((FRAMES, 200), np.float16))
    s = net.self_repair_vector(layer)
    if layer in DEAD:
        assert np.all(s[DEAD[layer][1]] == -np.float32(K10)) and np.all(s[SAT[layer][1]] == np.float32(K10))
    assert np.count_nonzero(s) >= 2, "the layer has no dead or saturated unit on this data"
    p = net.get_params()
    W1 = p[layer + ".LinearW"].astype(np.float16).astype(np.float64)
    W2 = p[layer + ".AffineW"].astype(np.float16).astype(np.float64)
    ref = sr.tdnnf_response(net.read_activation(below).astype(np.float64), W1, W2, s, 3)
    for key, want in ref.items():
        e = rel_fro(g[f"{layer}.{key}"].reshape(want.shape), want)
        print(f"{layer}.{key}: rel-Frobenius {e:.2e}")
        assert e <= GRAD_TOL, (key, e)
    net.close()


@pytest.mark.parametrize("frames", [300, 298], ids=["tail", "no-tail"])
def test_row_subsampled(gpu, frames):
    """KF_BN_ROWS_SUBSAMPLED: the statistics rows of a compact layer are its rows c < tc0; the tail
    rows and the scratch slot are neither counted nor repaired"""
    kf = gpu
    net = _net(kf, xcfg=tiny3_xcfg(), k=K10, rsub=True)
    net.set_sequences(_seq(frames))
    _, g = _step(kf, net, frames, og=_out_grad(frames, mod3=True))
    tc, tc0, rows = net.row_set()
    assert tc > 0 and tc0 == (frames - 1) // 3 + 1 and (tc > tc0) == (frames == 300)
    for name in SITES:
        compact = name.startswith(("tdnnf", "prefinal"))
        n = tc0 if compact else frames
        cnt, _, dsum = net.relu_stats_raw(name)
        assert cnt == n * HEIGHT.get(name, 1), name
        assert np.array_equal(dsum, _popcount(net, name, n)), name
    k16 = float(np.float16(K10))
    for layer in ("tdnnf6", "prefinal-chain"):
        pname, cols = DEAD[layer]
        want = -k16 * tc0                      # (with the tail rows repaired it would be -k16 tc)
        got = g[pname][0, cols].astype(np.float64)
        assert np.all(np.abs(got - want) <= GRAD_TOL * abs(want)), (layer, got, want)
    net.close()


def _snapshot(kf, net):
    out, g = _step(kf, net)
    acc = {n: net.batchnorm_stats(n, 0) for n in SITES}
    return out, g, acc


def _assert_same(a, b, what):
    assert np.array_equal(a[0].view(np.uint16), b[0].view(np.uint16)), what + ": output"
    for k in a[1]:
        assert np.array_equal(a[1][k].view(np.uint32), b[1][k].view(np.uint32)), f"{what}: gradient {k}"
    for n in a[2]:
        assert a[2][n][0] == b[2][n][0] and all(np.array_equal(x, y) for x, y in zip(a[2][n][1:], b[2][n][1:])), f"{what}: {n}"


def test_off_after_on_is_never_on_and_zero_scale_is_batchnorm_train(gpu):
    kf = gpu
    never = _net(kf, self_repair=False)
    base = _snapshot(kf, never)
    never.close()
    net = _net(kf, k=K10)
    on = _snapshot(kf, net)
    assert any(not np.array_equal(on[1][k], base[1][k]) for k in base[1]), "the switch changed no gradient"
    replay_net = _net(kf, k=K10)
    _assert_same(_snapshot(kf, replay_net), on, "a step replays")
    replay_net.close()
    net.set_self_repair(False)
    assert net.self_repair_sites() == []
    net.batchnorm_zero_stats()
    _assert_same(_snapshot(kf, net), base, "off after on")
    net.close()
    zero = _net(kf, k=0.0)
    _assert_same(_snapshot(kf, zero), base, "every scale 0")
    zero.close()


def test_accepted_without_a_site(gpu):
    kf = gpu
    base_net = _net(kf, bn_train=False, self_repair=False)
    base = _step(kf, base_net)
    base_net.close()
    net = _net(kf, bn_train=False)                       # training-mode BatchNorm off
    assert net.self_repair_sites() == []
    got = _step(kf, net)
    assert np.array_equal(got[0], base[0]) and all(np.array_equal(got[1][k], base[1][k]) for k in base[1])
    net.close()
    net = _net(kf, sites="batchnorm")                    # a site set without such a layer
    assert net.self_repair_sites() == []
    net.close()


def test_refusals_in_both_orders(gpu):
    """MXFP8, implicit dz, data parallel and nnet_backward_n beside self-repair, with the table's
    texts: whichever of two switches is set second, the refusal names self-repair. The switch counts
    from the moment it is set on a net with a layer it can govern, training-mode BatchNorm on or not."""
    kf = gpu
    from kfp16 import KfError, dp
    og = kf.upload_fp16(_out_grad(FRAMES))
    comm = dp.Communicator(0, 1, dp.unique_id(), 0)
    on = "with ReLU self-repair on \\(nnet_set_self_repair\\)"
    others = [(lambda n: n.set_fp8(True), "set_fp8: not supported " + on + "",
               "set_self_repair: not supported in MXFP8 mode \\(nnet_set_fp8\\)"),
              (lambda n: n.set_implicit_dz(True), "set_implicit_dz: not supported " + on + "",
               "set_self_repair: not supported with implicit dz \\(nnet_set_implicit_dz\\)"),
              (lambda n: n.bind_dp(comm, 1 << 20), "bind_dp: not supported " + on + ": the unit statistics would be each rank's own",
               "set_self_repair: not supported on a net bound to data parallel \\(nnet_bind_dp\\): the unit statistics would be "
               "each rank's own")]
    for bn_train in (True, False):
        for turn_on, second_text, first_text in others:
            # self-repair first: the other mode is refused, and stays off
            net = _net(kf, bn_train=bn_train)
            with pytest.raises(KfError, match=second_text):
                turn_on(net)
            net.close()
        if bn_train:
            continue
        for turn_on, second_text, first_text in others:
            # the other mode first (training-mode BatchNorm cannot be on beside it): self-repair is refused, and stays off
            net = _net(kf, bn_train=False, self_repair=False)
            turn_on(net)
            with pytest.raises(KfError, match=first_text):
                net.set_self_repair(True)
            net.set_self_repair(False)
            net.close()
    net = _net(kf)
    _step(kf, net, backward=False)
    with pytest.raises(KfError, match="backward_n: not supported " + on + ""):
        kf.check(kf.nnet.nnet_backward_n(net.h, og.ptr, 100), "nnet_backward_n")
    net.set_self_repair(False)
    with pytest.raises(KfError, match="backward_n: not supported with training-mode BatchNorm on"):
        kf.check(kf.nnet.nnet_backward_n(net.h, og.ptr, 100), "nnet_backward_n")
    net.close()
    comm.close()


# ---------------------------------------------------------------------------
# the whole step against the staged reference (tests/self_repair_ref.py SelfRepairOracle)
# ---------------------------------------------------------------------------
ACT_TOL = 2e-3
TOP = ["tdnnf5", "tdnnf6", "tdnnf7", "tdnnf8", "prefinal-l", "prefinal-chain", "output"]


def _reference_compare(kf, frames, sites, rsub):
    """forward, statistics and every gradient at k = 2^-10 against the staged reference with the
    GPU's ReLU decisions replayed; rsub: the row-subsampled step against BnRowsOracle plus the term
    on the rows 0 (mod 3), compared on the rows test_gpu_bn_rows.py compares"""
    import oracle  # noqa: F401
    import bn_rows_ref as rr
    import bn_sites_ref as bs
    import test_gpu_bn_rows as tbr
    from kfp16 import synth
    xcfg = tiny3_xcfg() if rsub else synth.load_xconfig("tiny.xconfig")
    site_list = ["tdnnf", "conv", "prefinal", "batchnorm"] if sites == "all" else sites.split(",")
    feats, og = _features(frames), _out_grad(frames, mod3=rsub)
    net = _net(kf, xcfg=xcfg, bn_train=False, self_repair=False, sites=sites, rsub=rsub)
    tp = {n: synth.trunc_fp16(v) for n, v in net.get_params().items()}
    net.close()
    probe = kf.Network(xcfg, max_frames=FRAMES)
    _, bns0 = synth.init_network(probe)
    probe.close()
    bns = bs.matched_bns(xcfg, tp, bns0, feats.astype(np.float32), site_list, threads=16)
    net = _net(kf, xcfg=xcfg, bn_train=False, self_repair=False, sites=sites, rsub=rsub)
    for (name, which), (m, v, g, b) in bns.items():
        net.set_bn(name, which, m, v, g, b, eps=1e-3)
    net.set_sequences(_seq(frames))
    net.set_batchnorm_train(True)
    net.set_self_repair(True)
    site_names = net.self_repair_sites()
    for name in site_names:
        net.set_self_repair_opts(name, K10)
    fb = kf.upload_fp16(feats)
    net.forward(fb.ptr, frames)
    tc, tc0, rows = net.row_set()
    assert (tc > 0) == rsub
    if rsub:
        exact = np.concatenate([np.arange(tc0), np.arange(tc0 + tbr.EXACT_TAIL, tc)]).astype(np.int64)
    names = TOP if rsub else SITES + ["prefinal-l", "output"]
    acts = {n: net.read_activation(n).astype(np.float32) for n in names}
    gov = tbr._governed(net)
    gov = [k for k in gov if not k[0].endswith("batchnorm")]
    stats = {k: net.batchnorm_batch_stats(*k) for k in gov}
    relu = net.relu_masks()
    counts = {n: net.relu_stats_raw(n) for n in site_names}
    gb = kf.upload_fp16(og[rows] if rsub else og)
    net.backward(gb.ptr)
    grads = net.read_grads()
    svec = {n: net.self_repair_vector(n) for n in site_names}
    net.close()

    S = rr.rows_mod3(frames) if rsub else None
    inner = sr.SelfRepairOracle(xcfg, tp, bns, site_list, threads=16, rows=S)
    ref = rr.BnRowsOracle(inner) if rsub else inner
    ref.forward(feats.astype(np.float32))
    worst = 0.0
    for n in names:
        e = rel_fro(acts[n][exact], ref.act(n)[rows[exact]]) if rsub else rel_fro(acts[n], ref.act(n))
        worst = max(worst, e / ACT_TOL)
        assert e <= ACT_TOL, (n, e)
    for key in gov:
        want = inner.stats[key]
        em, ev = tbr._stat_errors(key, stats[key], want)
        worst = max(worst, em / ACT_TOL, ev / ACT_TOL)
        assert em <= ACT_TOL and ev <= ACT_TOL, (key, em, ev)
    # The unit statistics against the reference's own decisions on the statistics rows: printed, not
    # bounded. A count moves by one for every element whose pre-activation lies within the forward
    # error of zero, and one count is 1 / n = 3.3e-3 of deriv_avg at n = 300, above the 2e-3 the
    # continuous statistics are held to. The decisions are replayed below for that reason, and the
    # counts are then held exactly.
    own = {n: np.asarray(m).copy() for n, m in inner.masks.items()}
    for n in site_names:
        H = HEIGHT.get(n, 1)
        m = own[n].reshape(frames, -1)
        if rsub:
            m = m[S]
        want = m.reshape(m.shape[0] * H, -1).sum(0).astype(np.float64)
        assert counts[n][0] == m.shape[0] * H, n
        print("%s: deriv_sum against the reference's own decisions, rel-Frobenius %.2e, largest column difference %d"
              % (n, rel_fro(counts[n][2], want), int(np.max(np.abs(counts[n][2] - want)))))
    # the GPU's ReLU decisions replayed (on the compared rows of the set), the term from their counts
    force = {}
    for n, m in own.items():
        w = m.size // frames
        if rsub and n in TOP:
            mm = m.reshape(frames, w).copy()
            mm[rows[exact]] = relu[n][:tc * w].reshape(tc, w)[exact]
            force[n] = mm.reshape(-1)
        else:
            force[n] = relu[n]
    ref.forward(feats.astype(np.float32), force_masks=force)
    for n in site_names:
        H = HEIGHT.get(n, 1)
        m = np.asarray(inner.masks[n]).reshape(frames, -1)
        if rsub:
            m = m[S]
        pop = m.reshape(m.shape[0] * H, -1).sum(0).astype(np.float64)
        # the statistics of the reference with the decisions replayed, restricted to the statistics rows: exact
        assert np.array_equal(counts[n][2], pop), n
        inner.repair[n] = sr.repair_vector(m.shape[0] * H, pop, K10)
        assert np.array_equal(inner.repair[n], svec[n]), n
        if n in DEAD:
            assert np.all(svec[n][DEAD[n][1]] == -np.float32(K10)) and np.all(svec[n][SAT[n][1]] == np.float32(K10))
    want = ref.backward(og.astype(np.float32))
    inner.close()
    errs = {n: rel_fro(grads[n], want[n]) for n in want}
    print("worst forward error / tolerance %.2f; grad errors: %s" % (worst, ", ".join(f"{n}={v:.2e}" for n, v in errs.items())))
    assert set(errs) == set(grads)
    bad = {n: v for n, v in errs.items() if v > GRAD_TOL}
    assert not bad, bad


def test_step_against_staged_reference(gpu):
    _reference_compare(gpu, FRAMES, "all", False)


@pytest.mark.parametrize("frames", [300, 298], ids=["tail", "no-tail"])
def test_row_subsampled_step_against_staged_reference(gpu, frames):
    _reference_compare(gpu, frames, "tdnnf,prefinal", True)


def test_loss_scale(gpu):
    """S = 4096: the repair vector is 4096 k, and the update agrees with the unscaled step's"""
    kf = gpu
    deltas = []
    for S in (None, 4096.0):
        net = _net(kf, k=1e-5)
        og = _out_grad(FRAMES).astype(np.float32)
        if S:
            net.set_loss_scale(True, init_scale=S, growth_interval=1 << 30)
            og = og * S
        p0 = net.get_params()
        _step(kf, net, og=og.astype(np.float16))
        s = net.self_repair_vector("tdnnf6")
        assert np.all(s[DEAD["tdnnf6"][1]] == -np.float32(np.float32(1e-5) * np.float32(S or 1.0)))
        net.update(1e-2, 0.0, 2.0, 1.0)
        p1 = net.get_params()
        deltas.append({k: p1[k].astype(np.float64) - p0[k] for k in p0})
        net.close()
    for k, d in deltas[0].items():
        assert rel_fro(deltas[1][k], d) <= GRAD_TOL, (k, rel_fro(deltas[1][k], d))


# ---------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def egs(tmp_path_factory):
    import egs_writer as W
    from kfp16 import egs, synth
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, 4, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    d = tmp_path_factory.mktemp("sr")
    W.write_ark(d / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(d / "cegs.*.ark"), batch_size=4).next_batch()
    return batch, synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)


@pytest.mark.parametrize("natural_gradient", [False, True], ids=["plain", "ng"])
def test_trainer(gpu, egs, natural_gradient):
    from kfp16 import synth, trainer
    kw = dict(learning_rate=1e-2, momentum=0.9, kaldi_update=True, max_param_change=2.0, orthonormal_every=2,
              dropout_schedule="0,0.3@0.5,0", total_steps=3, xent_regularize=0.1, row_subsampling=True,
              batchnorm_train=True, batchnorm_train_sites="all", batchnorm_train_rows="subsampled", self_repair=True,
              natural_gradient=natural_gradient, loss_scale=0.0 if natural_gradient else 4096.0)
    tr = trainer.EgsTrainer(synth.load_xconfig("tiny_xent.xconfig"), egs[1], max_egs=8, max_frames=800,
                            config=trainer.TrainConfig(**kw))
    synth.init_network(tr.net)
    for _ in range(3):
        tr.step(egs[0])
    assert np.isfinite(tr.result().objf)
    summary = tr.relu_summary()
    assert list(summary) == tr.net.self_repair_sites() and len(summary) >= 3
    for name, st in summary.items():
        assert st["count"] > 0 and 0 <= st["dead"] and 0 <= st["saturated"] and st["dead"] + st["saturated"] <= st["units"]
        assert st["units"] == tr.net._bn_dim(name, 0) and len(st["deriv_avg_pct"]) == 3
        d = tr.net.relu_stats(name)["deriv_avg"]
        o = tr.net.self_repair_opts(name)
        assert st["dead"] == int(np.sum(d <= o["lower"])) and st["saturated"] == int(np.sum(d > o["upper"]))
        assert st["deriv_avg_pct"][0] <= st["deriv_avg_pct"][1] <= st["deriv_avg_pct"][2]
    tr.net.close()


def test_trainer_needs_batchnorm_train():
    from kfp16 import trainer
    with pytest.raises(ValueError, match="self_repair needs batchnorm_train"):
        trainer.TrainConfig(self_repair=True, batchnorm_train=False)
