"""The Kaldi-style parameter update on the GPU: kf_update_maxchange (kf_ops.h) on a synthetic
flat buffer, nnet_update (kf_nnet.h) on tiny.xconfig, and the trainer's switch.

The reference is `ref_update` below: the rule of kf_ops.h restated in float64 numpy on the
float32 inputs the kernel is given. It is never compared with kf_sgd_flat or with the kernel
itself. Bounds:
  * stats (n_c, s_c, N, S): 1e-5 relative. d^2 is summed in fp32 over at most 16 elements per
    thread, a 64-lane tree and 4 waves (a 4096-element chunk), the chunks' sums in double:
    about (16 + 6 + 2) roundings of 2^-24 on a sum of positive terms, < 2e-6 on the square.
  * v: 2 ulp of fp32 (the kernel sums the three terms in double and rounds once).
  * w32: 1 ulp(w32) + 1e-5 |S s_c d_i| (the scales' error acts on the step, the final
    rounding on the weight).
  * w16 == rne_fp16(the stored w32), bit for bit; two runs bit-identical.
Every case asserts that no threshold (n_c against max_change_c, N against max_param_change)
lies within 1e-4 relative of its limit, so the bound on the norms cannot flip a decision.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ float64 reference
def ref_update(w, g, v, comps, lr, mom, mpc, l2_scale):
    """comps: [(segments [(b, e)], max_change, l2, lr_factor)], float32 values; w, g, v float32
    arrays. Returns w, v (float64, untouched outside the segments), the step S s_c d (float64),
    stats = (n_c, s_c, N, S) and the smallest relative distance of a norm from its limit."""
    w, g, v = w.astype(F64), g.astype(F64), v.astype(F64)
    lr, mom, mpc, l2_scale = F64(F32(lr)), F64(F32(mom)), F64(F32(mpc)), F64(F32(l2_scale))
    d, norms, scales = {}, [], []
    margin = np.inf
    for ci, (segs, mc, l2, lrf) in enumerate(comps):
        idx = np.concatenate([np.arange(b, e) for b, e in segs])
        mc, l2, lrf = F64(F32(mc)), F64(F32(l2)), F64(F32(lrf))
        v[idx] = mom * v[idx] + g[idx] + l2_scale * l2 * w[idx]
        d[ci] = (idx, lr * lrf * v[idx])
        n = np.sqrt(np.sum(d[ci][1] ** 2))
        if mc > 0:
            margin = min(margin, abs(n / mc - 1))
        norms.append(n)
        scales.append(mc / n if (mc > 0 and n > mc) else 1.0)
    norms, scales = np.array(norms), np.array(scales)
    N = np.sqrt(np.sum((scales * norms) ** 2))
    if mpc > 0:
        margin = min(margin, abs(N / mpc - 1))
    S = mpc / N if (mpc > 0 and N > mpc) else 1.0
    step = np.zeros_like(w)
    for ci, (idx, dd) in d.items():
        step[idx] = S * scales[ci] * dd
    return w - step, v, step, (norms, scales, N, S), margin


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F32))).astype(F64)


def check_against_ref(out, ref, covered, what=""):
    """out: (w32, w16 bits, v, stats array) of the GPU; ref: ref_update's result"""
    w32, w16, v, stats = out
    w_ref, v_ref, step, (norms, scales, N, S), margin = ref
    assert margin > 1e-4, f"{what}: a norm lies within 1e-4 of its limit ({margin:.2e}): the case decides nothing"
    nc = len(norms)
    got = np.concatenate([stats[:nc], stats[nc:2 * nc], stats[2 * nc:]]).astype(F64)
    want = np.concatenate([norms, scales, [N, S]])
    assert np.all(np.isfinite(got)), (what, got)
    err = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
    print(f"{what}: stats max rel err {err.max():.2e}; S {S:.4g}, clipped {int((scales < 1).sum())} of {nc}")
    assert err.max() <= 1e-5, (what, err, got, want)
    ev = np.abs(v.astype(F64) - v_ref)[covered] / ulp32(v_ref)[covered]
    print(f"{what}: v max err {ev.max():.2f} ulp")
    assert ev.max() <= 2.0, (what, ev.max())
    ew = np.abs(w32.astype(F64) - w_ref)[covered]
    bound = (ulp32(w32) + 1e-5 * np.abs(step))[covered]
    print(f"{what}: w32 max err / bound {np.max(ew / bound):.3f}")
    assert np.all(ew <= bound), (what, np.max(ew / bound))
    assert np.array_equal(w16[covered], w32[covered].astype(np.float16).view(np.uint16)), what
    assert np.all(np.isfinite(w32[covered])) and np.all(np.isfinite(v[covered]))


# ------------------------------------------------------------------ kernel level
SENT32, SENT16 = F32(-7.25e11), np.float16(-1234.0)


def _tables(kf, comps):
    """the device tables of kf_ops.h from [(segments, max_change, l2, lr_factor)]"""
    segs, cs, wg = [], [], 0
    for ci, (ss, mc, l2, lrf) in enumerate(comps):
        first = wg
        for b, e in ss:
            segs.append((b, e, ci, wg))
            wg += -(-(e - b) // kf.UPD_CHUNK)
        cs.append((mc, l2, lrf, first, wg - first))
    sa = (kf.KfUpdSegment * len(segs))(*[kf.KfUpdSegment(*s) for s in segs])
    ca = (kf.KfUpdComp * len(cs))(*[kf.KfUpdComp(*c) for c in cs])

    def up(arr):
        buf = kf.DeviceBuffer(C.sizeof(arr))
        kf.check(kf.core.bridge_transfer_int32(buf.ptr, C.addressof(arr), C.sizeof(arr) // 4), "tables")
        return buf
    return up(sa), len(segs), up(ca), len(cs)


class Flat:
    """device copies of a flat parameter set and one kf_update_maxchange call on them"""

    def __init__(self, kf, n, comps):
        self.kf, self.n, self.comps = kf, n, comps
        self.segs, self.nseg, self.cbuf, self.ncomp = _tables(kf, comps)
        sb = kf.core.kf_update_scratch_bytes(n, self.nseg, self.ncomp)
        assert sb > 0
        self.scratch = kf.DeviceBuffer(sb)
        self.stats = kf.DeviceBuffer((2 * self.ncomp + 2) * 4)

    def load(self, w, w16, g, v):
        kf = self.kf
        self.w, self.g, self.v = kf.upload_f32(w), kf.upload_f32(g), kf.upload_f32(v)
        self.h = kf.upload_fp16(w16)

    def set_grad(self, g):
        self.g = self.kf.upload_f32(g)

    def run(self, lr, mom, mpc, l2_scale):
        kf = self.kf
        kf.check(kf.core.kf_update_maxchange(self.w.ptr, self.h.ptr, self.g.ptr, self.v.ptr, self.n, self.segs.ptr,
                                             self.nseg, self.cbuf.ptr, self.ncomp, float(lr), float(mom), float(mpc),
                                             float(l2_scale), self.scratch.ptr, self.stats.ptr), "kf_update_maxchange")
        return (kf.read_f32(self.w.ptr, (self.n,)), kf.read_fp16(self.h.ptr, (self.n,)).view(np.uint16),
                kf.read_f32(self.v.ptr, (self.n,)), kf.read_f32(self.stats.ptr, (2 * self.ncomp + 2,)))


N_FLAT = 200064
# (segments, what the component is there for); the gaps between them are padding
LAYOUT = [
    ([(0, 70001)], "one long segment: 18 workgroups, a ragged tail, a length that is no multiple of 4"),
    ([(70019, 75019), (75072, 87417)], "two segments around padding, the first from an odd offset"),
    ([(87424, 87425)], "one element"),
    ([(87488, 90488)], "all-zero gradient, weights and velocity"),
    ([(90496, 99496)], "max_change 0 under a huge gradient"),
    ([(99520, 119520)], "just under its limit"),
    ([(119552, 200003)], "the rest, with an L2 term and a learning-rate factor"),
]


@pytest.fixture(scope="module")
def flat_inputs():
    rng = np.random.default_rng(2024)
    n = N_FLAT
    w = (rng.standard_normal(n) * 0.1).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    g2 = rng.standard_normal(n).astype(F32)
    v = (rng.standard_normal(n) * 0.5).astype(F32)
    covered = np.zeros(n, bool)
    for segs, _ in LAYOUT:
        for b, e in segs:
            assert not covered[b:e].any()
            covered[b:e] = True
    b, e = LAYOUT[3][0][0]
    w[b:e] = 0
    g[b:e] = 0
    g2[b:e] = 0
    v[b:e] = 0
    b, e = LAYOUT[4][0][0]
    g[b:e] *= 1e4
    g2[b:e] *= 1e4
    w16 = w.astype(np.float16)
    w[~covered], v[~covered], w16[~covered] = SENT32, SENT32, SENT16
    g[~covered] = np.nan          # the padding of the gradient is not read either
    g2[~covered] = np.nan
    for a in (w, g, g2, v, w16, covered):
        a.setflags(write=False)
    return dict(w=w, g=g, g2=g2, v=v, w16=w16, covered=covered)


LR, MOM, L2S = 1e-3, 0.9, 8.0


def _flat_comps(inp):
    """max-changes from the float64 norms of the first call with no limits at all: components
    0 and 1 clip (limits at 50 % and 80 % of their norms), 5 stays 0.1 % under its limit"""
    opts = [(0.0, 0.01, 1.0), (0.0, 0.0, 0.5), (0.0, 0.0, 1.0), (0.0, 0.02, 1.0), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0),
            (0.0, 0.005, 0.333)]
    free = [(segs, *o) for (segs, _), o in zip(LAYOUT, opts)]
    norms = ref_update(inp["w"], np.nan_to_num(inp["g"]), inp["v"], free, LR, MOM, 0.0, L2S)[3][0]
    mc = [0.5 * norms[0], 0.8 * norms[1], 0.75, 0.75, 0.0, 1.001 * norms[5], 1.5 * norms[6]]
    return [(segs, F32(m), F32(o[1]), F32(o[2])) for (segs, _), o, m in zip(LAYOUT, opts, mc)]


@pytest.mark.parametrize("mpc", [2.0, 1e7, 0.0], ids=["global-binds", "global-loose", "global-off"])
def test_kernel_two_calls_against_float64(gpu, flat_inputs, mpc):
    kf, inp = gpu, flat_inputs
    comps = _flat_comps(inp)
    cov = inp["covered"]
    fl = Flat(kf, N_FLAT, comps)
    fl.load(inp["w"], inp["w16"], inp["g"], inp["v"])
    out1 = fl.run(LR, MOM, mpc, L2S)
    ref1 = ref_update(inp["w"], np.nan_to_num(inp["g"]), inp["v"], comps, LR, MOM, mpc, L2S)
    check_against_ref(out1, ref1, cov, "call 1")
    norms, scales, N, S = ref1[3]
    assert scales[0] < 1 and scales[1] < 1 and scales[5] == 1 and scales[6] == 1   # clipped / just under
    assert norms[2] > 0 and scales[2] in (1.0, 0.75 / norms[2])                    # the 1-element component
    assert norms[3] == 0 and scales[3] == 1 and out1[3][3] == 0 and out1[3][7 + 3] == 1  # zero norm: scale 1
    assert scales[4] == 1 and norms[4] > 100 and N >= norms[4]                    # unclipped, counted in N
    assert (S < 1) == (mpc == 2.0)
    # the padding is neither read (NaN gradient) nor written
    assert np.all(out1[0][~cov] == SENT32) and np.all(out1[2][~cov] == SENT32)
    assert np.all(out1[1][~cov] == np.array([SENT16]).view(np.uint16)[0])
    # the second call: momentum acts on the stored velocity
    fl.set_grad(inp["g2"])
    out2 = fl.run(LR, MOM, mpc, L2S)
    ref2 = ref_update(out1[0], np.nan_to_num(inp["g2"]), out1[2], comps, LR, MOM, mpc, L2S)
    check_against_ref(out2, ref2, cov, "call 2")
    assert np.all(out2[0][~cov] == SENT32) and np.all(out2[2][~cov] == SENT32)
    v_nomom = ref_update(out1[0], np.nan_to_num(inp["g2"]), np.zeros(N_FLAT, F32), comps, LR, MOM, mpc, L2S)[1]
    assert np.max(np.abs(out2[2][cov] - v_nomom[cov])) > 0.1                       # the velocity was used


def test_kernel_runs_are_bit_identical(gpu, flat_inputs):
    kf, inp = gpu, flat_inputs
    comps = _flat_comps(inp)
    outs = []
    for _ in range(2):
        fl = Flat(kf, N_FLAT, comps)
        fl.load(inp["w"], inp["w16"], inp["g"], inp["v"])
        fl.run(LR, MOM, 2.0, L2S)
        fl.set_grad(inp["g2"])
        outs.append(fl.run(LR, MOM, 2.0, L2S))
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint32 if a.dtype == F32 else a.dtype),
                              b.view(np.uint32 if b.dtype == F32 else b.dtype))


def test_kernel_without_limits_is_plain_sgd(gpu, flat_inputs):
    """All limits 0, l2 0, factors 1: w32 agrees with the float64 rule w - lr (mom v + g) to 1 ulp.
    The inputs keep |w| in [0.5, 2] and |lr v| < 0.1, so the roundings of v (0.5 ulp(v) * lr) and
    of the product lr * v stay below 0.1 ulp(w) beside the final rounding's 0.5 ulp(w)."""
    kf, inp = gpu, flat_inputs
    rng = np.random.default_rng(5)
    cov = inp["covered"]
    w = (rng.uniform(0.5, 2.0, N_FLAT) * rng.choice([-1.0, 1.0], N_FLAT)).astype(F32)
    g = np.clip(rng.standard_normal(N_FLAT), -4, 4).astype(F32)
    v = np.clip(rng.standard_normal(N_FLAT), -4, 4).astype(F32)
    comps = [(segs, F32(0), F32(0), F32(1)) for segs, _ in LAYOUT]
    fl = Flat(kf, N_FLAT, comps)
    fl.load(w, w.astype(np.float16), g, v)
    lr, mom = F32(0.01), F32(0.9)
    w32, w16, vv, stats = fl.run(lr, mom, 0.0, 123.0)
    v_ref = F64(mom) * v.astype(F64) + g.astype(F64)
    w_ref = w.astype(F64) - F64(lr) * v_ref
    assert np.all(stats[7:14] == 1) and stats[15] == 1
    err = (np.abs(w32.astype(F64) - w_ref) / ulp32(w_ref))[cov]
    print(f"plain SGD: w32 max err {err.max():.3f} ulp")
    assert err.max() <= 1.0
    assert np.max((np.abs(vv.astype(F64) - v_ref) / ulp32(v_ref))[cov]) <= 2.0
    assert np.array_equal(w16[cov], w32[cov].astype(np.float16).view(np.uint16))
    assert np.array_equal(w32[~cov], w[~cov]) and np.array_equal(vv[~cov], v[~cov])


def test_kernel_rejects_bad_arguments(gpu, flat_inputs):
    kf = gpu
    fl = Flat(kf, N_FLAT, _flat_comps(flat_inputs))
    fl.load(flat_inputs["w"], flat_inputs["w16"], flat_inputs["g"], flat_inputs["v"])
    with pytest.raises(kf.KfError):
        fl.run(LR, MOM, -1.0, L2S)
    assert kf.core.kf_update_scratch_bytes(-1, 1, 1) == -1
    fl.run(LR, MOM, 2.0, L2S)   # and the stream is still healthy


# ------------------------------------------------------------------ network level
T_NET = 120
KEYS = {"cnn1": "max-change=0.5 l2-regularize=0.002 learning-rate-factor=0.5",
        "tdnnf6": "l2-regularize=0.01", "prefinal-l": "max-change=0", "output": "learning-rate-factor=2"}
MPC, NET_L2S, NET_MOM = 2.0, 40.0, 0.9


def _net_xconfig(synth):
    lines = []
    for ln in synth.load_xconfig("tiny.xconfig").splitlines():
        for name, keys in KEYS.items():
            if f"name={name} " in ln:
                ln += " " + keys
        lines.append(ln)
    return "\n".join(lines) + "\n"


def _net_comps(net):
    out = []
    for c in net.components():
        segs = [(net.params[t][2], net.params[t][2] + net.params[t][0] * net.params[t][1]) for t in c["tensors"]]
        out.append((segs, c["max_change"], c["l2"], c["lr_factor"]))
    return out


def _net_case(kf, fp8):
    from kfp16 import synth
    xcfg = _net_xconfig(synth)
    net = kf.Network(xcfg, max_frames=T_NET)
    synth.init_network(net, seed=11)
    if fp8:
        net.set_fp8(True)
    feats = kf.upload_fp16(synth.make_features(T_NET, 40, seed=5))
    net.forward(feats.ptr, T_NET)
    out0 = net.read_activation("output")
    og = (np.random.default_rng(7).standard_normal(out0.shape) * 0.05).astype(np.float16)
    gb = kf.upload_fp16(og)
    net.backward(gb.ptr)
    w0 = kf.read_f32(net.master_ptr, (net.num_params,))
    g = kf.read_f32(net.grad_ptr, (net.num_params,))
    comps = _net_comps(net)
    covered = np.zeros(net.num_params, bool)
    for segs, *_ in comps:
        for b, e in segs:
            covered[b:e] = True
    # lr from the float64 reference at lr = 1 (norms are linear in lr): between the points where
    # the third- and the fourth-smallest n_c / max_change_c reach 1, so all but three of the
    # limited components clip
    v0 = np.zeros(net.num_params, F32)
    norms1 = ref_update(w0, g, v0, comps, 1.0, NET_MOM, 0.0, NET_L2S)[3][0]
    ratios = sorted(n / mc for n, (_, mc, _, _) in zip(norms1, comps) if mc > 0)
    lr = F32(1.0 / np.sqrt(ratios[2] * ratios[3]))
    ref = ref_update(w0, g, v0, comps, lr, NET_MOM, MPC, NET_L2S)
    return dict(net=net, xcfg=xcfg, feats=feats, out0=out0, w0=w0, g=g, comps=comps, covered=covered,
                lr=lr, ref=ref)


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16", "fp8"])
def test_network_update_against_float64(gpu, fp8):
    kf = gpu
    from kfp16 import synth
    c = _net_case(kf, fp8)
    net, ref, cov = c["net"], c["ref"], c["covered"]
    norms, scales, N, S = ref[3]
    assert int((scales < 1).sum()) >= 2 and S < 1, (scales, N, S)       # the case does clip, twice over
    assert scales[[x["name"] for x in net.components()].index("prefinal-l")] == 1   # max-change=0: no limit
    net.update(c["lr"], NET_MOM, MPC, NET_L2S)
    st = net.update_stats()
    stats = np.concatenate([st["norms"], st["scales"], [st["global_norm"], st["global_scale"]]]).astype(F32)
    w32 = kf.read_f32(net.master_ptr, (net.num_params,))
    named = net.get_params()
    assert np.array_equal(net.flat_params(named)[cov], w32[cov])
    w16 = kf.read_fp16(kf.nnet.nnet_weight_buffer(net.h), (net.num_params,)).view(np.uint16)
    # the velocity buffer has no accessor: v is checked at kernel level, here through w32 (the
    # step is lr lrf v); the reference's own v stands in for it in the shared check
    check_against_ref((w32, w16, ref[1].astype(F32), stats), ref, cov, "fp8 net" if fp8 else "net")
    assert np.array_equal(w32[~cov], c["w0"][~cov])                      # padding untouched
    # the next forward runs on the new weights
    net.forward(c["feats"].ptr, T_NET)
    out1 = net.read_activation("output")
    assert not np.array_equal(out1.view(np.uint16), c["out0"].view(np.uint16))
    fresh = kf.Network(c["xcfg"], max_frames=T_NET)
    synth.init_network(fresh, seed=11)
    # set_params(updated) gives the fresh network the masters; its fp16 copy is then the updated
    # network's, bit for bit, written through nnet_weight_buffer: set_params itself truncates
    # fp32 to fp16 and flushes fp16 subnormals, where the update rounds to nearest
    fresh.set_params(fresh.unflatten(w32))
    kf.check(kf.core.bridge_transfer_fp16(kf.nnet.nnet_weight_buffer(fresh.h), w16.ctypes.data, w16.size), "w16")
    fresh.weights_changed()
    if fp8:
        fresh.set_fp8(True)
    fresh.forward(c["feats"].ptr, T_NET)
    assert np.array_equal(fresh.read_activation("output").view(np.uint16), out1.view(np.uint16))
    if fp8:
        # and equals the forward after nnet_weights_changed on the same weights
        net.weights_changed()
        net.forward(c["feats"].ptr, T_NET)
        assert np.array_equal(net.read_activation("output").view(np.uint16), out1.view(np.uint16))
    fresh.close()
    net.close()


def test_network_update_options_take_effect_and_momentum_carries(gpu):
    """nnet_set_component_opts after an update re-uploads the table; the second update uses
    the first one's velocity."""
    kf = gpu
    c = _net_case(kf, False)
    net, cov = c["net"], c["covered"]
    lr = c["lr"]
    net.update(lr, NET_MOM, MPC, NET_L2S)
    w1 = kf.read_f32(net.master_ptr, (net.num_params,))
    v1 = c["ref"][1]            # float64 velocity of the first call (g + l2 term, from zero)
    net.set_component_opts("tdnnf7.affine", 0.05, 0.0, 1.0)
    comps = _net_comps(net)
    i7 = [x["name"] for x in net.components()].index("tdnnf7.affine")
    assert comps[i7][1] == F32(0.05)
    net.update(lr, NET_MOM, 0.0, NET_L2S)
    st = net.update_stats()
    ref = ref_update(w1, c["g"], v1.astype(F32), comps, lr, NET_MOM, 0.0, NET_L2S)
    norms, scales, N, S = ref[3]
    assert ref[4] > 1e-4 and S == 1 and scales[i7] < 1
    got = np.concatenate([st["norms"], st["scales"], [st["global_norm"], st["global_scale"]]]).astype(F64)
    want = np.concatenate([norms, scales, [N, S]])
    # v1 enters as float32(the float64 reference), within 2 ulp of the kernel's stored one: 2e-7
    # relative on the step, far inside the 1e-5 of both bounds
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-5
    assert abs(st["scales"][i7] * st["norms"][i7] - 0.05) <= 1e-5 * 0.05
    w2 = kf.read_f32(net.master_ptr, (net.num_params,))
    ew = np.abs(w2.astype(F64) - ref[0])[cov]
    assert np.all(ew <= (ulp32(w2) + 1e-5 * np.abs(ref[2]))[cov])
    net.close()


# ------------------------------------------------------------------ trainer
def test_trainer_default_is_todays_sgd_and_kaldi_update_opts_in(gpu, tmp_path):
    """kaldi_update=False (the default), whatever the new fields hold: a step's parameters are
    bit-identical to forward / objective / backward / Network.sgd done by hand.
    kaldi_update=True: Network.update ran (its report exists and respects the limits)."""
    kf = gpu
    import egs_writer as W
    from kfp16 import chain, egs, synth, trainer
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, 4, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=4).next_batch()
    den = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)
    xcfg = synth.load_xconfig("tiny.xconfig")
    lr, mom = 1e-3, 0.9

    def flat(net):
        return kf.read_f32(net.master_ptr, (net.num_params,)).view(np.uint32)

    tr = trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=800,
                            config=trainer.TrainConfig(learning_rate=lr, momentum=mom, max_param_change=2.0,
                                                       l2_scale=5.0))
    assert tr.cfg.kaldi_update is False
    synth.init_network(tr.net)
    tr.step(batch)
    tr.result()
    # by hand
    net = kf.Network(xcfg, max_frames=800)
    synth.init_network(net)
    T = batch.total_frames
    fbuf = kf.DeviceBuffer(800 * 40 * 2)
    batch.features_to_device(fbuf.ptr, 40)
    net.forward(fbuf.ptr, T)
    obj = chain.Chain(chain.DenGraph(den), max_seqs=8, max_frames=800 // 3 + 1)
    row0, frames = trainer.chain_rows(batch.frame_offsets, batch.num_frames, batch.frames_per_seq, 3, 30)
    g = kf.DeviceBuffer(T * 200 * 2)
    kf.core.bridge_gpu_memset(g.ptr, 0, T * 200 * 2)
    obj.compute(chain.NumBatch(batch.num_fsts()), net.activation("output")[0], 200, T, row0, frames, 3, g.ptr, 200)
    net.backward(g.ptr)
    net.sgd(lr, mom)
    kf.sync()
    assert np.array_equal(flat(tr.net), flat(net))

    tk = trainer.EgsTrainer(xcfg, den, max_egs=8, max_frames=800,
                            config=trainer.TrainConfig(learning_rate=lr, momentum=mom, kaldi_update=True,
                                                       max_param_change=1e-6))
    synth.init_network(tk.net)
    tk.step(batch)
    tk.result()
    st = tk.net.update_stats()
    assert st["global_scale"] < 1 and abs(st["global_scale"] * st["global_norm"] - 1e-6) <= 1e-5 * 1e-6
    assert not np.array_equal(flat(tk.net), flat(tr.net))
    net.close()
