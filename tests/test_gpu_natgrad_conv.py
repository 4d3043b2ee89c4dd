"""Natural gradient on the parameter side of the conv components on the GPU: the kf_ng_conv_*
kernels (kf_ops.h, csrc/natgrad_conv.hip) on a synthetic table, nnet_set_natural_gradient_conv on
tiny.xconfig and the row-subsampled cnn_tdnn_17f, the guards and EgsTrainer.

The reference is tests/natgrad_conv_ref.py (float64, checked on its own). Bounds.
  * L and trX of both sides: 1e-6 rel-Frobenius: accumulated in double from fp32 inputs and rounded
    once to fp32 (6e-8), with headroom.
  * G^ against gamma_in gamma_out (I - W_in^T W_in) G (I - W_out^T W_out) with the W and gamma read
    back: 1e-5, DESIGN §20's bound for gradient agreement.
  * JT, gamma and the state after the update (rho', d', W'^T W') against the float64 reference fed
    the unrounded statistics: 4 x the worst deviation seen on the MI355X over the cases below
    (SEEN), the convention of test_gpu_natgrad.test_state_against_float64.
"""
import ctypes as C

import numpy as np
import pytest

import natgrad_conv_ref as CR
import natgrad_ref as R
from test_gpu_natgrad import SENT32, Pres, _component_tensors, _flat_grad, _gext, _gext_of, _upload_table

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
# worst relative deviations seen on the MI355X: JT, gamma, rho', d', W'^T W'. (W'^T W' is that large in
# one case only, the in side of 577 x 64 from the initial state: 64 rows of data for rank 80, so 16
# eigenvalues sit on the floor and their rows of W' are the statistics' rounding over the floor; 2.7e-6
# is the worst of the other cases.)
SEEN = (2.41e-7, 1.22e-7, 2.44e-7, 3.41e-6, 6.21e-2)
BOUND = tuple(4.0 * x for x in SEEN)
SHAPES = [(9, 16, 1), (54, 48, 1), (577, 64, 1), (2304, 256, 1), (54, 48, 0)]
CASES = [(K, N, b, warm) for K, N, b in SHAPES for warm in (0, 5)]
IDS = [f"{K}x{N}{'_bias' if b else ''}_t{w}" for K, N, b, w in CASES]


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, F64) - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def conv_runs(gpu):
    """all the cases as one table: statistics (updating), scales, apply and state, twice from the same inputs"""
    kf = gpu
    rng = np.random.default_rng(61)
    refs, dims, comps, grads, off = [], [], [], [], 12
    for K, N, bias, warm in CASES:
        Din = K + bias
        ref = CR.ConvPre(Din, N)
        # low rank on both sides: a low_rank_batch in the span of basis, spread over the rows by left
        basis, left = np.linalg.qr(rng.standard_normal((N, 6)))[0].T, np.linalg.qr(rng.standard_normal((Din, 6)))[0]
        for s in range(warm + 1):
            G = left @ R.low_rank_batch(rng, 6, N, basis, 0.0) + 0.02 * rng.standard_normal((Din, N))
            if s < warm:
                ref.step(G)
        grads.append(G.astype(F32))
        idx = []
        for p in (ref.pin, ref.pout):
            idx.append(len(dims) if p is not None else -1)
            if p is not None:
                dims.append((p.D, p.R))
        comps.append(kf.KfNgComp(off, off + K * N + 64 if bias else -1, K, N, idx[0], idx[1]))
        off += K * N + 64 + (N + 64 if bias else 0)
        refs.append(ref)
    n = off + 20
    g0 = np.full(n, SENT32, F32)
    cov = np.zeros(n, bool)
    for c, G in zip(comps, grads):
        g0[c.dw_off:c.dw_off + c.K * c.N] = G[:c.K].reshape(-1)
        cov[c.dw_off:c.dw_off + c.K * c.N] = True
        if c.db_off >= 0:
            g0[c.db_off:c.db_off + c.N] = G[c.K]
            cov[c.db_off:c.db_off + c.N] = True
    ps = Pres(kf, dims)
    table = (kf.KfNgComp * len(comps))(*comps)
    tdev = _upload_table(kf, table)
    targs = (C.addressof(table), tdev.ptr, len(comps)) + ps.args()
    sb = kf.core.kf_ng_conv_scratch_bytes(C.addressof(table), len(comps), C.addressof(ps.table), len(dims))
    assert sb > 0
    scratch = kf.DeviceBuffer(sb)
    outs = []
    for _ in range(2):
        ps.set_state([p for ref in refs for p in ref.sides()])   # (rounds the references' W to fp32)
        ps.stat = kf.upload_f32(np.zeros(ps.nst, F32))
        g = kf.upload_f32(g0)
        kf.check(kf.core.kf_ng_conv_stats(g.ptr, n, *targs, ps.w32.ptr, 4.0, 1, ps.stat.ptr, scratch.ptr), "kf_ng_conv_stats")
        assert np.array_equal(kf.read_f32(g.ptr, (n,)).view(np.uint32), g0.view(np.uint32))
        rep = ps.scales().copy()
        kf.check(kf.core.kf_ng_conv_apply(g.ptr, n, *targs, ps.w32.ptr, ps.report.ptr, scratch.ptr), "kf_ng_conv_apply")
        stat = ps.read_stat()
        ps.state(1)
        outs.append(dict(g=kf.read_f32(g.ptr, (n,)), stat=stat, rep=rep, state=ps.read(),
                         flags=kf.read_f32(ps.report.ptr, (len(dims), kf.NG_REPORT))[:, 4].copy()))
    before = [[None if p is None else p.copy() for p in (ref.pin, ref.pout)] for ref in refs]
    steps = [ref.step(G.astype(F64)) for ref, G in zip(refs, grads)]
    return dict(kf=kf, ps=ps, comps=comps, refs=refs, before=before, steps=steps, g0=g0, cov=cov, outs=outs)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_kernels_against_float64(conv_runs, i):
    a, kf = conv_runs, conv_runs["kf"]
    c, out = a["comps"][i], a["outs"][0]
    (got, _) = out["state"]
    _, info = a["steps"][i]
    assert (c.pre_in >= 0) == (CASES[i][0] + CASES[i][2] >= 16) and c.pre_out >= 0
    worst, proj, gam = np.zeros(5), [None, None], [1.0, 1.0]
    for side, (name, pi) in enumerate((("in", c.pre_in), ("out", c.pre_out))):
        if pi < 0:
            continue
        p, st, bef, aft = a["ps"].table[pi], info[name], a["before"][i][side], (a["refs"][i].pin, a["refs"][i].pout)[side]
        Rp, o = kf.ng_rp(p.R), kf.ng_stat_offsets(p.D, p.R)
        s = out["stat"][p.st_off:p.st_off + o["floats"]]
        L = s[o["L"]:o["L"] + Rp * Rp].reshape(Rp, Rp)
        JT = s[o["JT"]:o["JT"] + p.D * Rp].reshape(p.D, Rp)
        assert not L[p.R:].any() and not L[:, p.R:].any() and not JT[:, p.R:].any()
        assert s[1] == st["N"] and s[2] == 4.0 * st["N"] and out["flags"][pi] == 0
        e_l, e_t = _rel(L[:p.R, :p.R], st["L"]), abs(F64(s[0]) - st["trx"]) / st["trx"]
        gam[side], proj[side] = F64(out["rep"][pi][0]), bef.proj()
        g = got[pi]
        dev = np.array([_rel(JT[:, :p.R], st["J"].T), abs(gam[side] - st["gamma"]) / st["gamma"],
                        abs(g["rho"] - aft.rho) / aft.rho, np.max(np.abs(g["d"] - aft.d) / aft.d),
                        _rel(g["W"].astype(F64).T @ g["W"].astype(F64), aft.proj())])
        print(f"{IDS[i]} {name}: D {p.D} R {p.R} gamma {gam[side]:.4f}; rel dev L {e_l:.2e} trX {e_t:.2e} JT {dev[0]:.2e} "
              f"gamma {dev[1]:.2e} rho' {dev[2]:.2e} d' {dev[3]:.2e} W'^T W' {dev[4]:.2e}")
        assert e_l <= 1e-6 and e_t <= 1e-6 and g["t"] == bef.t + 1
        worst = np.maximum(worst, dev)
    want = R.precondition_gradient(_gext(a["g0"], c), gam[0], gam[1], proj[0], proj[1])
    err = _rel(_gext(out["g"], c), want)
    print(f"{IDS[i]}: G^ rel-Frobenius {err:.2e}; worst (JT, gamma, rho', d', W'^T W') {worst}")
    assert err <= 1e-5 and (not CASES[i][3] or max(gam) > 1.15)   # the warm state has a real scale
    assert np.all(worst <= BOUND), worst


def test_kernels_touch_nothing_else_and_are_deterministic(conv_runs):
    a = conv_runs
    o1, o2 = a["outs"]
    assert np.array_equal(o1["g"][~a["cov"]].view(np.uint32), a["g0"][~a["cov"]].view(np.uint32))
    assert np.all(np.isfinite(o1["g"][a["cov"]])) and not np.array_equal(o1["g"][a["cov"]], a["g0"][a["cov"]])
    for k in ("g", "stat", "rep"):
        assert np.array_equal(o1[k].view(np.uint32), o2[k].view(np.uint32)), k
    for x, y in zip(o1["state"][1], o2["state"][1]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("xconfig, T, rsub", [("tiny.xconfig", 300, False), ("cnn_tdnn_17f.xconfig", 600, True)],
                         ids=["tiny_all_rows", "17f_row_subsampled"])
def test_network_two_sided_identity(gpu, xconfig, T, rsub):
    kf = gpu
    from kfp16 import synth
    net = kf.Network(synth.load_xconfig(xconfig), max_frames=T)
    synth.init_network(net, seed=12)
    if rsub:
        net.set_row_subsampling(3)
    feats = kf.upload_fp16(synth.make_features(T, 40, seed=4))
    net.forward(feats.ptr, T)
    out = net.read_activation("output")
    og = kf.upload_fp16((np.random.default_rng(8).standard_normal(out.shape) * 0.05).astype(np.float16))
    net.backward(og.ptr)
    G = _flat_grad(kf, net)
    tensors = _component_tensors(net)
    convs = {c["name"] for c in net.components() if c["name"].startswith("cnn")}
    assert convs
    runs = {}
    for conv in (False, True):
        net.set_natural_gradient(True, conv=conv)
        for step in range(6):
            state = net.natural_gradient_state() if step in (0, 5) else None
            net.forward(feats.ptr, T)
            net.backward(og.ptr)
            if state is not None:
                runs[conv, step] = (state, net.natural_gradient_stats(), _flat_grad(kf, net))
    conv_el = np.zeros(net.num_params, bool)
    for step in (0, 5):
        state, stats, Gh = runs[True, step]
        assert all(s["t"] == step for s in state) and not any(r["flag"] for r in stats)
        by = {}
        for s, r in zip(state, stats):
            assert (s["name"], s["side"]) == (r["name"], r["side"])
            if s["name"] in convs:
                by.setdefault(s["name"], {})[s["side"]] = (s["W"].astype(F64), F64(r["gamma"]))
        assert set(by) == convs, sorted(by)
        for name, sides in by.items():
            dw, db = tensors[name]
            win, gin = sides.get("in", (None, 1.0))
            wout, gout = sides.get("out", (None, 1.0))
            want = R.precondition_gradient(_gext_of(net, G, dw, db), gin, gout, None if win is None else win.T @ win,
                                           None if wout is None else wout.T @ wout)
            err = _rel(_gext_of(net, Gh, dw, db), want)
            print(f"t={step} {name}: G {want.shape} gamma {gin:.4f} {gout:.4f} rel-Frobenius {err:.2e}")
            assert err <= 1e-5, (step, name, err)
            assert step < 5 or all(g > 1.0 for _, g in sides.values())
            for t in (dw, db):
                r, c, off = net.params[t]
                conv_el[off:off + r * c] = True
        # everything but the conv components: bit-equal to natural gradient without the opt-in
        assert np.array_equal(Gh[~conv_el].view(np.uint32), runs[False, step][2][~conv_el].view(np.uint32))
        assert not any(s["name"] in convs for s in runs[False, step][0])
    net.close()


def test_guards(gpu):
    kf = gpu
    from kfp16 import dp, synth
    net = kf.Network(synth.load_xconfig("tiny.xconfig"), max_frames=150)
    synth.init_network(net, seed=3)
    with pytest.raises(kf.KfError, match="natural gradient is off"):
        kf.check(kf.nnet.nnet_set_natural_gradient_conv(net.h, 1, None), "nnet_set_natural_gradient_conv")
    net.set_fp8(True)
    with pytest.raises(kf.KfError, match="MXFP8"):
        net.set_natural_gradient(True, conv=True)
    net.set_fp8(False)
    comm = dp.Communicator(0, 1, dp.unique_id(), 0)
    net.bind_dp(comm, 1 << 20)
    with pytest.raises(kf.KfError, match="data parallel"):
        net.set_natural_gradient(True, conv=True)
    net.bind_dp(None, 0)
    net.set_natural_gradient(True, conv=True, conv_opts=dict(rank_in=16))
    assert any(s["name"].startswith("cnn") and s["W"].shape[0] <= 16 for s in net.natural_gradient_state())
    with pytest.raises(kf.KfError, match="natural gradient"):
        net.set_fp8(True)
    with pytest.raises(kf.KfError, match="natural gradient"):
        net.bind_dp(comm, 1 << 20)
    with pytest.raises(kf.KfError, match="bad options"):
        net.set_natural_gradient(True, conv=True, conv_opts=dict(num_minibatches_history=0.0))
    net.set_natural_gradient(False)
    assert net.natural_gradient_state() == []
    comm.close()
    net.close()


def test_trainer(gpu, tmp_path):
    """two steps with natural_gradient_conv; with it False, the gradient of a trainer built without the field"""
    kf = gpu
    import egs_writer as W
    from kfp16 import egs, synth, trainer
    exs, _ = W.make_egs(np.random.default_rng(31), 4, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=4).next_batch()
    den = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)
    assert trainer.TrainConfig().natural_gradient_conv is False
    grads = []
    for kw in (dict(natural_gradient_conv=True), dict(natural_gradient_conv=False), dict()):
        tr = trainer.EgsTrainer(synth.load_xconfig("tiny.xconfig"), den, max_egs=8, max_frames=800,
                                config=trainer.TrainConfig(learning_rate=1e-3, momentum=0.9, kaldi_update=True,
                                                           max_param_change=1.0, natural_gradient=True, **kw))
        synth.init_network(tr.net)
        tr.step(batch)
        assert np.isfinite(tr.result().objf)
        grads.append(_flat_grad(kf, tr.net))
        if kw.get("natural_gradient_conv"):
            tr.step(batch)
            rep = tr.net.natural_gradient_stats()
            assert np.isfinite(tr.result().objf) and not any(r["flag"] for r in rep)
            assert any(r["name"].startswith("cnn") for r in rep) and all(np.isfinite(r["gamma"]) for r in rep)
        tr.net.close()
    assert np.array_equal(grads[1].view(np.uint32), grads[2].view(np.uint32))
