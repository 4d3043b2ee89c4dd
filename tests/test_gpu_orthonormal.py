"""The semi-orthogonal constraint on the GPU: kf_orthonormal_constrain (kf_ops.h) on a synthetic
flat buffer, nnet_constrain_orthonormal (kf_nnet.h) on tiny.xconfig, and the trainer's schedule.

The reference is tests/ortho_ref.py ref_constrain: the rule of kf_ops.h restated in float64
numpy on the float32 inputs the kernel is given (checked on its own in
tests/test_orthonormal_ref.py). It is never compared with the kernel's own output path.

Bounds of the one-step comparison (ortho_ref.kernel_bounds, from the kernel's accumulation
lengths; u = 2^-24, A = |W|^T |W|, all terms reference quantities, none fitted to the GPU):
  * P_ij: an fp32 fma chain over at most 512 rows of W (one chunk) plus the chunks' partials
    added in fp32: dP_ij <= (min(K, 512) + chunks) u A_ij.
  * tP, tPP are summed in double from that P: dtP <= sum dP_ii, dtPP <= sum (2 |P| dP + dP^2);
    s^2 = tPP / tP so e2 = d(s^2) / s^2 <= dtPP / tPP + dtP / tP, ds / s <= e2 / 2 + u,
    dratio / ratio <= dtPP / tPP + 2 dtP / tP + u (fixed scale: s exact, ratio 1).
  * Q = P - s^2 I rounded to fp32: dQ <= dP + I s^2 e2 + u |Q|; |d err| <= |dQ|_F + u err.
  * w32: W Q is an fp32 fma chain over n, the factor is rounded to fp32:
    dw <= f (|W| dQ + n u |W| |Q|) + (e2 + 2 u) |X| + 1 ulp(w32).
  * nu matches exactly: every case first asserts that the reference ratio lies at least 1e-3
    relative away from 1.02 and from 1.1 (and that the bound on ratio is below that), so no
    rounding can flip a decision.
  * w16 == rne_fp16(the stored w32), bit for bit; two runs bit-identical.
Convergence is a property: after 12 calls err / (s^2 sqrt(n)) <= 1e-4 in float64 on the returned
w32 (the reference reaches < 1e-12, fp32 floors near 1e-6) and |W|_F moves by less than 2 %.

Mutations of csrc/orthonormal.hip, each run once on the MI355X against this file: see DESIGN §19.
"""
import ctypes as C

import numpy as np
import pytest

import ortho_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT32, SENT16 = F32(-7.25e11), np.float16(-1234.0)


# ------------------------------------------------------------------ kernel level
class Flat:
    """a poisoned flat buffer holding the given matrices [(K, n, c, w float32 [K, n])] at odd
    offsets with sentinel padding between and after them, and kf_orthonormal_constrain on it"""

    def __init__(self, kf, mats, check_table=True):
        self.kf, self.mats = kf, mats
        off, self.offs = 12, []
        for K, n, c, w in mats:
            self.offs.append(off)
            off += K * n + 20 + 4 * (len(self.offs) % 3)      # gaps of 20 / 24 / 28 elements
        self.n = off + 36
        self.w0 = np.full(self.n, SENT32, F32)
        self.covered = np.zeros(self.n, bool)
        for (K, n, c, w), o in zip(mats, self.offs):
            self.w0[o:o + K * n] = np.asarray(w, F32).reshape(-1)
            if c != 0:
                self.covered[o:o + K * n] = True
        # the fp16 buffer goes in poisoned everywhere: the Gram must not read it
        self.h0 = np.full(self.n, SENT16, np.float16)
        self.table = (kf.KfOrthoMat * len(mats))(*[kf.KfOrthoMat(o, K, n, c, 0)
                                                   for (K, n, c, w), o in zip(mats, self.offs)])
        self.sb = kf.core.kf_orthonormal_scratch_bytes(C.addressof(self.table), len(mats))
        if check_table:
            assert self.sb > 0
        self.tdev = kf.DeviceBuffer(C.sizeof(self.table))
        kf.check(kf.core.bridge_transfer_int32(self.tdev.ptr, C.addressof(self.table), C.sizeof(self.table) // 4), "table")
        self.scratch = kf.DeviceBuffer(max(self.sb, 256))
        self.stats = kf.upload_f32(np.full(4 * len(mats), SENT32, F32))
        self.load(self.w0)

    def load(self, w):
        self.w, self.h = self.kf.upload_f32(w), self.kf.upload_fp16(self.h0)

    def call(self):
        return self.kf.core.kf_orthonormal_constrain(self.w.ptr, self.h.ptr, self.n, C.addressof(self.table),
                                                     self.tdev.ptr, len(self.mats), self.scratch.ptr, self.stats.ptr)

    def read(self):
        kf = self.kf
        return (kf.read_f32(self.w.ptr, (self.n,)), kf.read_fp16(self.h.ptr, (self.n,)).view(np.uint16),
                kf.read_f32(self.stats.ptr, (4 * len(self.mats),)).reshape(-1, 4))

    def run(self):
        self.kf.check(self.call(), "kf_orthonormal_constrain")
        return self.read()

    def mat(self, flat, i):
        K, n = self.mats[i][:2]
        return flat[self.offs[i]:self.offs[i] + K * n].reshape(K, n)


# (K, n, c, seed): the smallest; the tiny net's shapes; K and n multiples of neither 64 nor 128;
# a bench shape; Q larger than LDS; the largest; a fixed scale; one that is off
SHAPES = [(32, 32, -1.0, 1), (256, 64, -1.0, 2), (512, 64, -1.0, 3), (416, 96, -1.0, 4), (3072, 160, -1.0, 5),
          (1536, 256, -1.0, 6), (6144, 320, -1.0, 7), (512, 64, 0.5, 8), (64, 32, 0.0, 9)]


def _gauss_mats():
    out = []
    for K, n, c, seed in SHAPES:
        w = R.gaussian(np.random.default_rng(1000 + seed), K, n)
        if c > 0:
            w = (F32(c) * w).astype(F32)     # near its target scale (tests/test_orthonormal_ref.py)
        out.append((K, n, c, w))
    return out


@pytest.fixture(scope="module")
def gauss(gpu):
    """one call on all the shapes together, a second from the same inputs, and the references"""
    kf = gpu
    mats = _gauss_mats()
    fl = Flat(kf, mats)
    out1 = fl.run()
    fl.load(fl.w0)
    out2 = fl.run()
    refs = [R.ref_constrain(w, c) for K, n, c, w in mats]
    return dict(fl=fl, mats=mats, out=out1, out2=out2, refs=refs)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[f"{K}x{n}_c{c:g}" for K, n, c, _ in SHAPES])
def test_kernel_one_step_against_float64(gauss, i):
    fl, (K, n, c, w), r = gauss["fl"], gauss["mats"][i], gauss["refs"][i]
    w32, w16, stats = gauss["out"]
    got, goth = fl.mat(w32, i), fl.mat(w16, i)
    s, ratio, err, nu = (F64(x) for x in stats[i])
    if c == 0:
        assert np.array_equal(got.view(np.uint32), np.asarray(w, F32).view(np.uint32))      # bit-untouched
        assert np.all(goth == SENT16.view(np.uint16)) and not stats[i].any()
        return
    assert r["margin"] > 1e-3, f"ratio {r['ratio']:.5f} lies within 1e-3 of a threshold: the case decides nothing"
    ds, dratio, derr, dw = R.kernel_bounds(w, c, r)
    assert dratio < 1e-3 * r["ratio"]
    print(f"{K}x{n} c={c:g}: ref s {r['s']:.6f} ratio {r['ratio']:.5f} err {r['err']:.5f} nu {r['nu']}; "
          f"got/bound: s {abs(s - r['s']) / ds:.3f} ratio {abs(ratio - r['ratio']) / max(dratio, 1e-300):.3f} "
          f"err {abs(err - r['err']) / derr:.3f} w32 {np.max(np.abs(got.astype(F64) - r['w']) / dw):.3f}")
    assert nu == r["nu"]
    assert abs(s - r["s"]) <= ds and abs(err - r["err"]) <= derr
    assert abs(ratio - r["ratio"]) <= dratio
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got.astype(F64) - r["w"]) <= dw)
    assert np.array_equal(goth, got.astype(np.float16).view(np.uint16))


def test_kernel_touches_nothing_else_and_is_deterministic(gauss):
    fl = gauss["fl"]
    w32, w16, stats = gauss["out"]
    cov = fl.covered
    assert np.array_equal(w32[~cov].view(np.uint32), fl.w0[~cov].view(np.uint32))            # padding, the off matrix
    assert np.all(w16[~cov] == SENT16.view(np.uint16))
    assert not np.any(w32[cov] == SENT32)
    for a, b in zip(gauss["out"], gauss["out2"]):
        assert np.array_equal(a.view(np.uint32 if a.dtype == F32 else a.dtype), b.view(np.uint32 if b.dtype == F32 else b.dtype))


def test_kernel_exact_cases(gpu):
    kf = gpu
    rng = np.random.default_rng(21)
    p1, p2 = R.perm_columns(rng, 128, 64), R.perm_columns(rng, 160, 96)
    fl = Flat(kf, [(128, 64, 1.0, 2 * p1), (160, 96, -1.0, p2), (64, 32, -1.0, np.zeros((64, 32), F32)),
                   (128, 64, -1.0, 3 * p1)])
    w32, w16, stats = fl.run()
    # P = 4 I, Q = 3 I, the factor is 0.5: exactly -W / 2
    # (compared as values: the zeros come back as +0 where -W / 2 would carry -0)
    assert np.array_equal(fl.mat(w32, 0), -p1)
    assert np.array_equal(stats[0], np.array([1.0, 1.0, np.sqrt(F64(9 * 64)), 0.125], F32))
    # permutation columns with the floating scale: a fixed point
    assert np.array_equal(fl.mat(w32, 1).view(np.uint32), p2.view(np.uint32))
    assert np.array_equal(stats[1], np.array([1.0, 1.0, 0.0, 0.125], F32))
    # all-zero: untouched, s = 0, no NaN
    assert not fl.mat(w32, 2).any() and np.all(fl.mat(w16, 2) == SENT16.view(np.uint16))
    assert np.array_equal(stats[2], np.zeros(4, F32))
    # a scaled fixed point of the floating scale: s = 3
    assert np.array_equal(fl.mat(w32, 3).view(np.uint32), (3 * p1).view(np.uint32))
    assert np.array_equal(stats[3], np.array([3.0, 1.0, 0.0, 0.125], F32))
    for i in (0, 1, 3):
        assert np.array_equal(fl.mat(w16, i), fl.mat(w32, i).astype(np.float16).view(np.uint16))
    assert np.array_equal(w32[~fl.covered].view(np.uint32), fl.w0[~fl.covered].view(np.uint32))


def test_kernel_converges(gpu):
    """12 calls on the K >= 4 n shapes: semi-orthogonal to fp32's floor, the norm kept"""
    kf = gpu
    mats = [(K, n, c, w) for K, n, c, w in _gauss_mats() if K >= 4 * n and c != 0]
    assert len(mats) >= 6
    fl = Flat(kf, mats)
    for _ in range(12):
        kf.check(fl.call(), "kf_orthonormal_constrain")
    w32, w16, stats = fl.read()
    for i, (K, n, c, w) in enumerate(mats):
        got = fl.mat(w32, i)
        e = R.rel_err(got, c)
        growth = np.linalg.norm(got.astype(F64)) / np.linalg.norm(w.astype(F64))
        print(f"{K}x{n} c={c:g}: err / (s^2 sqrt n) {R.rel_err(w, c):.3e} -> {e:.3e}, |W|_F x {growth:.5f}")
        assert e <= 1e-4
        if c < 0:
            assert abs(growth - 1) < 0.02
    assert np.array_equal(w16[fl.covered], w32[fl.covered].astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("K, n", [(32, 64), (96, 48), (40, 32), (1088, 544)],
                         ids=["n_gt_K", "n_48", "K_40", "n_544"])
def test_kernel_rejects_unsupported_shapes(gpu, K, n):
    kf = gpu
    rng = np.random.default_rng(K)
    good = R.gaussian(rng, 64, 32)
    fl = Flat(kf, [(64, 32, -1.0, good), (K, n, -1.0, R.gaussian(rng, K, n))], check_table=False)
    assert fl.sb == -1
    assert fl.call() == -1                                          # before anything is launched
    assert b"transposed case not supported" in kf.core.kf_last_error()
    kf.sync()
    w32, w16, stats = fl.read()
    assert np.array_equal(w32.view(np.uint32), fl.w0.view(np.uint32)) and np.all(w16 == SENT16.view(np.uint16))
    assert np.all(stats == SENT32)
    # the same shape with c = 0 is no error: it is not looked at
    fl2 = Flat(kf, [(64, 32, -1.0, good), (K, n, 0.0, R.gaussian(rng, K, n))])
    w32, _, stats = fl2.run()
    assert np.array_equal(fl2.mat(w32, 1).view(np.uint32), fl2.mat(fl2.w0, 1).view(np.uint32))
    assert not np.array_equal(fl2.mat(w32, 0), good) and not stats[1].any()


def test_kernel_rejects_a_matrix_outside_the_buffer(gpu):
    kf = gpu
    fl = Flat(kf, [(64, 32, -1.0, R.gaussian(np.random.default_rng(1), 64, 32))])
    fl.n -= 100                                                     # the matrix now ends past n_params
    assert fl.call() == -1
    fl.n += 100
    kf.sync()
    assert np.array_equal(fl.read()[0].view(np.uint32), fl.w0.view(np.uint32))


# ------------------------------------------------------------------ network level
T_NET = 120
CONSTRAINED = {"tdnnf5.linear": "tdnnf5.LinearW", "tdnnf6.linear": "tdnnf6.LinearW", "tdnnf7.linear": "tdnnf7.LinearW",
               "tdnnf8.linear": "tdnnf8.LinearW", "prefinal-chain.linear": "prefinal-chain.SmallW"}


def _w16(kf, net):
    return kf.read_fp16(kf.nnet.nnet_weight_buffer(net.h), (net.num_params,)).view(np.uint16)


def _velocity(kf, net):
    """the velocity buffer has no accessor: with zero weights and a zero gradient, nnet_sgd at
    lr = 1, momentum = 1 leaves w32 = -v exactly"""
    kf.core.bridge_gpu_memset(net.master_ptr, 0, net.num_params * 4)
    kf.core.bridge_gpu_memset(net.grad_ptr, 0, net.num_params * 4)
    net.sgd(1.0, 1.0)
    return -kf.read_f32(net.master_ptr, (net.num_params,))


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16", "fp8"])
def test_network_constrain_against_float64(gpu, fp8):
    kf = gpu
    from kfp16 import synth
    xcfg = synth.load_xconfig("tiny.xconfig")
    net = kf.Network(xcfg, max_frames=T_NET)
    synth.init_network(net, seed=15)
    if fp8:
        net.set_fp8(True)
    assert net.orthonormal_components() == list(CONSTRAINED)
    feats = kf.upload_fp16(synth.make_features(T_NET, 40, seed=5))
    # one training step first, so the velocity is not zero
    net.forward(feats.ptr, T_NET)
    out0 = net.read_activation("output")
    gb = kf.upload_fp16((np.random.default_rng(7).standard_normal(out0.shape) * 0.05).astype(np.float16))
    net.backward(gb.ptr)
    net.sgd(1e-4, 0.9)
    w0 = kf.read_f32(net.master_ptr, (net.num_params,))
    h0 = _w16(kf, net)
    named0 = net.get_params()
    net.forward(feats.ptr, T_NET)
    out1 = net.read_activation("output")

    net.constrain_orthonormal()
    st = net.orthonormal_stats()
    w1 = kf.read_f32(net.master_ptr, (net.num_params,))
    h1 = _w16(kf, net)
    assert st["names"] == list(CONSTRAINED)
    cov = np.zeros(net.num_params, bool)
    for k, (comp, tensor) in enumerate(CONSTRAINED.items()):
        rows, cols, off = net.params[tensor]
        cov[off:off + rows * cols] = True
        w = named0[tensor]
        assert np.array_equal(w.reshape(-1), w0[off:off + rows * cols]) and w.shape == (rows, cols)
        r = R.ref_constrain(w, -1.0)
        assert r["margin"] > 1e-3, (comp, r["ratio"])
        ds, dratio, derr, dw = R.kernel_bounds(w, -1.0, r)
        got = w1[off:off + rows * cols].reshape(rows, cols)
        print(f"{comp} {rows}x{cols}: ratio {r['ratio']:.4f} nu {r['nu']} w32 err / bound "
              f"{np.max(np.abs(got.astype(F64) - r['w']) / dw):.3f}")
        assert np.all(np.abs(got.astype(F64) - r["w"]) <= dw)
        assert not np.array_equal(got, w)
        assert abs(F64(st["scale"][k]) - r["s"]) <= ds and abs(F64(st["ratio"][k]) - r["ratio"]) <= dratio
        assert abs(F64(st["err"][k]) - r["err"]) <= derr
    # everything else, padding included, is bit-identical in both buffers
    assert np.array_equal(w1[~cov].view(np.uint32), w0[~cov].view(np.uint32))
    assert np.array_equal(h1[~cov], h0[~cov])
    assert np.array_equal(h1[cov], w1[cov].astype(np.float16).view(np.uint16))
    # the derived copies were refreshed: the next forward equals that of a fresh network given
    # the same fp16 weights through nnet_weight_buffer + nnet_weights_changed
    net.forward(feats.ptr, T_NET)
    out2 = net.read_activation("output")
    assert not np.array_equal(out2.view(np.uint16), out1.view(np.uint16))
    fresh = kf.Network(xcfg, max_frames=T_NET)
    synth.init_network(fresh, seed=15)
    fresh.set_params(fresh.unflatten(w1))
    kf.check(kf.core.bridge_transfer_fp16(kf.nnet.nnet_weight_buffer(fresh.h), h1.ctypes.data, h1.size), "w16")
    fresh.weights_changed()
    if fp8:
        fresh.set_fp8(True)
    fresh.forward(feats.ptr, T_NET)
    assert np.array_equal(fresh.read_activation("output").view(np.uint16), out2.view(np.uint16))
    fresh.close()
    # the velocity is not touched: it equals that of a twin that never ran the constraint
    twin = kf.Network(xcfg, max_frames=T_NET)
    synth.init_network(twin, seed=15)
    if fp8:
        twin.set_fp8(True)
    twin.forward(feats.ptr, T_NET)
    twin.backward(gb.ptr)
    twin.sgd(1e-4, 0.9)
    v_twin, v_net = _velocity(kf, twin), _velocity(kf, net)
    assert np.any(v_twin[cov] != 0) and np.array_equal(v_net.view(np.uint32), v_twin.view(np.uint32))
    twin.close()
    net.close()


def test_network_without_constrained_components_is_a_noop(gpu):
    kf = gpu
    from kfp16 import synth
    net = kf.Network(synth.load_xconfig("tiny.xconfig"), max_frames=T_NET)
    synth.init_network(net, seed=11)
    net.constrain_orthonormal()
    net.orthonormal_stats()
    for comp in CONSTRAINED:
        net.set_component_orthonormal(comp, 0.0)
    assert net.orthonormal_components() == []
    w0, h0 = kf.read_f32(net.master_ptr, (net.num_params,)), _w16(kf, net)
    assert kf.nnet.nnet_constrain_orthonormal(net.h) == 0
    kf.sync()
    assert np.array_equal(kf.read_f32(net.master_ptr, (net.num_params,)).view(np.uint32), w0.view(np.uint32))
    assert np.array_equal(_w16(kf, net), h0)
    with pytest.raises(kf.KfError, match="no nnet_constrain_orthonormal has run"):    # nothing was launched
        net.orthonormal_stats()
    # switched back on with a fixed scale: the table is rebuilt
    net.set_component_orthonormal("tdnnf6.linear", 1.0)
    net.constrain_orthonormal()
    st = net.orthonormal_stats()
    assert st["names"] == ["tdnnf6.linear"] and st["scale"][0] == 1.0 and st["ratio"][0] == 1.0
    assert not np.array_equal(kf.read_f32(net.master_ptr, (net.num_params,)), w0)
    net.close()


# ------------------------------------------------------------------ trainer
def test_trainer_schedule(gpu, tmp_path):
    """orthonormal_every = 2 over 4 steps: right after steps 2 and 4 tdnnf6.linear is closer to
    semi-orthogonal than without the constraint from the same seed; orthonormal_every = 0 is the
    default trainer bit for bit. The trainers use the Kaldi-style update, whose max-change bounds
    a step whatever the synthetic gradient's size (plain SGD at this rate diverges on it). Printed, not asserted: err / (s^2 sqrt n) of every constrained
    component under kaldi_update with orthonormal_every = 4, after every fourth step from 20 to 48."""
    kf = gpu
    import egs_writer as W
    from kfp16 import egs, synth, trainer
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, 4, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=4).next_batch()
    den = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)
    xcfg = synth.load_xconfig("tiny.xconfig")

    def make(**kw):
        tr = trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=800,
                                config=trainer.TrainConfig(learning_rate=1e-3, momentum=0.9, kaldi_update=True,
                                                           max_param_change=1.0, **kw))
        synth.init_network(tr.net)
        return tr

    def err6(tr):
        return R.rel_err(tr.net.get_params()["tdnnf6.LinearW"])

    assert trainer.TrainConfig().orthonormal_every == 0
    on, off, default = make(orthonormal_every=2), make(orthonormal_every=0), make()
    e_on, e_off = [], []
    for step in range(1, 5):
        for tr in (on, off, default):
            tr.step(batch)
            tr.result()
        e_on.append(err6(on))
        e_off.append(err6(off))
    print("tdnnf6.linear err / (s^2 sqrt n) per step, every 2:", e_on, "off:", e_off)
    assert e_on[1] < e_off[1] and e_on[3] < e_off[3]
    assert e_on[0] == e_off[0]                       # step 1: no constraint yet
    assert on.net.orthonormal_stats()["names"] == list(CONSTRAINED)

    def flat(tr):
        return kf.read_f32(tr.net.master_ptr, (tr.net.num_params,)).view(np.uint32)
    assert np.array_equal(flat(off), flat(default)) and not np.array_equal(flat(on), flat(off))
    for tr in (on, off, default):
        tr.net.close()

    tk = make(orthonormal_every=4)
    for step in range(1, 49):
        tk.step(batch)
        tk.result()
        if step >= 20 and step % 4 == 0:
            p = tk.net.get_params()
            print(f"kaldi_update, every 4, after step {step}:",
                  {c: f"{R.rel_err(p[t]):.2e}" for c, t in CONSTRAINED.items()})
    tk.net.close()
