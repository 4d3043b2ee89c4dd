"""Natural-gradient preconditioning on the GPU: the kf_ng_* kernels (kf_ops.h, csrc/natgrad.hip)
on synthetic tables, and nnet_set_natural_gradient (kf_nnet.h) on tiny.xconfig, on the row-subsampled
cnn_tdnn_17f and through EgsTrainer.

The reference is tests/natgrad_ref.py: DESIGN §20's rule restated in float64 numpy (checked on its
own in tests/test_natgrad_ref.py). It is never compared with the kernels' own output path.

Bounds.
  * State kernel: the solver works in double on fp32 inputs (L, JT, trX and W rounded to fp32, K
    formed in the kernel from that JT; the reference gets the unrounded statistics), so the bound is the fp32 input rounding as it
    passes through the update. Measured once on the MI355X over the cases below:
    the worst relative deviations were rho' STATE_SEEN[0], d' STATE_SEEN[1], W'^T W' STATE_SEEN[2];
    the test's bounds are 4 x those, for input variation (the kernels are deterministic).
  * Apply kernel and the network's identity with the plain gradient: rel-Frobenius 1e-5 against
    the float64 formula, the bound the project uses for gradient agreement; padding bit-unchanged;
    two runs bit-identical. (The in-side passes run in double: with fp32 chains the network case
    missed the bound where gamma_in exceeds about 12)
  * trX: 1e-6 relative against float64.
  * Network statistics: NET_SEEN below, measured once on the MI355X; they rest on the fp16 storage
    of H. gamma must stay within 1e-2, or H would have to be kept in fp32.
"""
import ctypes as C

import numpy as np
import pytest

import natgrad_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT32 = F32(-7.25e11)
# worst relative deviations seen on the MI355X (rho', d', W'^T W'); the bounds are 4 x these
STATE_SEEN = (1.95e-7, 5.03e-8, 1.95e-7)
STATE_BOUND = tuple(4.0 * x for x in STATE_SEEN)


def _opts(kf, **kw):
    o = kf.KfNgOpts()
    kf.core.kf_ng_default_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _upload_bytes(kf, arr):
    a = np.ascontiguousarray(arr)
    assert a.nbytes % 4 == 0
    buf = kf.DeviceBuffer(a.nbytes)
    kf.check(kf.core.bridge_transfer_int32(buf.ptr, a.ctypes.data, a.nbytes // 4), "upload")
    return buf


def _upload_table(kf, table):
    buf = kf.DeviceBuffer(C.sizeof(table))
    kf.check(kf.core.bridge_transfer_int32(buf.ptr, C.addressof(table), C.sizeof(table) // 4), "table")
    return buf


def _read_f64(kf, ptr, n):
    return kf.read_f32(ptr, (2 * n,)).view(F64)


class Pres:
    """a table of preconditioners [(D, R)] with its state, statistics, report and scratch buffers"""

    def __init__(self, kf, dims, **opts):
        self.kf, self.dims = kf, dims
        self.opts = _opts(kf, **opts)
        w = hh = s = st = 0
        rows = []
        for D, Rk in dims:
            rows.append(kf.KfNgPre(D, Rk, w, hh, s, st))
            w += kf.ng_rp(Rk) * D + 8                         # gaps: the state of one must not reach the next
            hh += kf.ng_rp(Rk) * (kf.ng_w16_ld(D) + 1) + 8
            s += 2 + kf.ng_rp(Rk)
            st += kf.ng_stat_offsets(D, Rk)["floats"] + 4
        self.nw, self.nh, self.ns, self.nst = w, hh, s, st
        self.table = (kf.KfNgPre * len(dims))(*rows)
        self.tdev = _upload_table(kf, self.table)
        self.w32 = kf.upload_f32(np.full(w, SENT32, F32))
        self.w16 = kf.upload_fp16(np.full(hh, -1234.0, np.float16))
        self.sc = _upload_bytes(kf, np.zeros(s, F64))
        self.stat_host = np.zeros(st, F32)
        self.stat = kf.upload_f32(self.stat_host)
        self.report = kf.upload_f32(np.full(kf.NG_REPORT * len(dims), SENT32, F32))
        sb = kf.core.kf_ng_state_scratch_bytes(C.addressof(self.table), len(dims))
        assert sb > 0
        self.scratch = kf.DeviceBuffer(sb)

    def args(self):
        return C.addressof(self.table), self.tdev.ptr, len(self.dims)

    def init(self):
        self.kf.check(self.kf.core.kf_ng_init(*self.args(), C.byref(self.opts), self.w32.ptr, self.w16.ptr, self.sc.ptr),
                      "kf_ng_init")

    def set_state(self, refs):
        """upload the references' states; their W is first rounded to what fp32 holds"""
        kf = self.kf
        w, w16, sc = np.full(self.nw, SENT32, F32), np.full(self.nh, -1234.0, np.float16), np.zeros(self.ns, F64)
        for p, ref in zip(self.table, refs):
            Rp = kf.ng_rp(p.R)
            ref.W = ref.W.astype(F32).astype(F64)
            m = np.zeros((Rp, p.D), F32)
            m[:p.R] = ref.W
            w[p.w_off:p.w_off + Rp * p.D] = m.reshape(-1)
            w16[p.h_off:p.h_off + Rp * (kf.ng_w16_ld(p.D) + 1)] = self.half_image(m)
            sc[p.s_off], sc[p.s_off + 1] = ref.rho, ref.t
            sc[p.s_off + 2:p.s_off + 2 + p.R] = ref.d
        self.w32, self.w16, self.sc = kf.upload_f32(w), kf.upload_fp16(w16), _upload_bytes(kf, sc)

    def half_image(self, m):
        """the fp16 copy of W [Rp x D] as kf_ops.h lays it out: rows padded to the pitch, then the
        last column once more"""
        Rp, D = m.shape
        img = np.zeros((Rp, self.kf.ng_w16_ld(D)), np.float16)
        img[:, :D] = m
        return np.concatenate([img.reshape(-1), m[:, D - 1].astype(np.float16)])

    def set_stats(self, stats):
        """stats: per preconditioner dict(L, J, trx, N) in float64, rounded to fp32 here (K = J J^T is
        the state kernel's own product)"""
        kf = self.kf
        h = np.zeros(self.nst, F32)
        for p, s in zip(self.table, stats):
            Rp, o = kf.ng_rp(p.R), kf.ng_stat_offsets(p.D, p.R)
            h[p.st_off], h[p.st_off + 1] = s["trx"], s["N"]
            m = np.zeros((Rp, Rp), F32)
            m[:p.R, :p.R] = s["L"]
            h[p.st_off + o["L"]:p.st_off + o["L"] + Rp * Rp] = m.reshape(-1)
            if s.get("J") is not None:
                jt = np.zeros((p.D, Rp), F32)
                jt[:, :p.R] = np.asarray(s["J"]).T
                h[p.st_off + o["JT"]:p.st_off + o["JT"] + p.D * Rp] = jt.reshape(-1)
        self.stat_host = h
        self.stat = kf.upload_f32(h)

    def read_stat(self):
        return self.kf.read_f32(self.stat.ptr, (self.nst,))

    def scales(self):
        kf = self.kf
        kf.check(kf.core.kf_ng_scales(*self.args(), C.byref(self.opts), self.sc.ptr, self.stat.ptr, self.report.ptr),
                 "kf_ng_scales")
        return kf.read_f32(self.report.ptr, (len(self.dims), kf.NG_REPORT))

    def state(self, update=1):
        kf = self.kf
        kf.check(kf.core.kf_ng_state(*self.args(), C.byref(self.opts), update, self.w32.ptr, self.w16.ptr, self.sc.ptr,
                                     self.stat.ptr, self.scratch.ptr, self.report.ptr), "kf_ng_state")

    def read(self):
        """per preconditioner (W [R x D] fp32, d, rho, t; the fp16 copy is checked against W here), and the raw buffers"""
        kf = self.kf
        w = kf.read_f32(self.w32.ptr, (self.nw,))
        h = kf.read_fp16(self.w16.ptr, (self.nh,))
        sc = _read_f64(kf, self.sc.ptr, self.ns)
        out = []
        for p in self.table:
            Rp = kf.ng_rp(p.R)
            m = w[p.w_off:p.w_off + Rp * p.D].reshape(Rp, p.D)
            mh = h[p.h_off:p.h_off + Rp * (kf.ng_w16_ld(p.D) + 1)]
            assert not m[p.R:].any()                                        # the padding rows stay zero
            assert np.array_equal(mh.view(np.uint16), self.half_image(m).view(np.uint16))
            out.append(dict(W=m[:p.R].copy(), d=sc[p.s_off + 2:p.s_off + 2 + p.R].copy(),
                            rho=sc[p.s_off], t=sc[p.s_off + 1]))
        return out, (w, h, sc)


# ------------------------------------------------------------------ init, scales
def test_default_init_and_scales(gpu):
    kf = gpu
    dims = [(97, 8), (321, 80), (3073, 20), (160, 80)]
    ps = Pres(kf, dims)
    ps.init()
    got, (w, h, sc) = ps.read()
    rng = np.random.default_rng(5)
    refs, stats = [], []
    for (D, Rk), g in zip(dims, got):
        ref = R.Pre(D, Rk)
        assert g["rho"] == ref.rho and np.array_equal(g["d"], ref.d) and g["t"] == 0
        assert np.allclose(g["W"], ref.W, rtol=3e-7, atol=0)
        ref.W = g["W"].astype(F64)
        X = rng.standard_normal((50, D))
        stats.append(ref.stats(X))
        refs.append(ref)
    # the gaps between the states are not written
    cov = np.zeros(ps.nw, bool)
    for p in ps.table:
        cov[p.w_off:p.w_off + kf.ng_rp(p.R) * p.D] = True
    assert np.all(w[~cov] == SENT32)
    covh = np.zeros(ps.nh, bool)
    for p in ps.table:
        covh[p.h_off:p.h_off + kf.ng_rp(p.R) * (kf.ng_w16_ld(p.D) + 1)] = True
    assert np.all(h[~covh] == np.float16(-1234.0))
    ps.set_stats(stats)
    rep = ps.scales()
    for ref, s, r in zip(refs, stats, rep):
        g = ref.gamma(s["trx"], np.diag(s["L"]))
        assert g > 1.0 and abs(r[0] - g) <= 1e-6 * g
        assert r[1] == F32(ref.rho) and abs(r[2] - ref.d.sum()) <= 1e-6 * ref.d.sum() and r[3] == 0 and r[4] == 0
    # a zero or non-finite trace gives gamma = 1
    for s, bad in zip(stats, (0.0, np.nan, np.inf, -1.0)):
        s["trx"] = bad
    ps.set_stats(stats)
    assert np.array_equal(ps.scales()[:, 0], np.ones(4, F32))


# ------------------------------------------------------------------ state kernel
STATE_N = 200
STATE_CASES = [(D, Rk, t) for Rk in (8, 32, 80) for D in (97, 321) for t in (0, 5)] + [(97, 16, "equal"), (97, 16, "floor")]


def _state_case(D, Rk, kind, seed):
    """the reference before the update, the statistics fed to both sides, and whether only
    W'^T W' can be compared (an eigenvalue gap below 1e-6)"""
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((D, 8)))[0].T
    ref = R.Pre(D, Rk)
    if kind in (5, "floor"):
        for _ in range(5):
            ref.step(R.low_rank_batch(rng, STATE_N, D, basis))
    ref.W = ref.W.astype(F32).astype(F64)
    if kind == "equal":
        # rows along an orthonormal set Q^T R_0 of R_0's row space, the first two equally strong,
        # and rows outside that space: Z = Q diag((a sigma_i^2 + b dr)^2) Q^T, not diagonal, with
        # one eigenvalue twice
        q = np.linalg.qr(rng.standard_normal((Rk, Rk)))[0]
        sigma = np.concatenate([[3.0, 3.0], np.linspace(2.0, 0.5, Rk - 2)])
        rt = ref.rt()
        out = rng.standard_normal((40, D))
        out -= (out @ rt.T) @ rt
        s = ref.stats(np.vstack([sigma[:, None] * (q.T @ rt), out]))
    elif kind == "floor":
        # statistics no data gives: a negative L on the last three directions takes their
        # eigenvalues below (rho (1 - eta))^2
        eta = ref.eta(STATE_N)
        e = ref.e()
        dr = ref.d + ref.rho
        L = 1e-3 * np.min(dr * e) * rng.standard_normal((Rk, Rk))
        L = 0.5 * (L + L.T)
        L[np.arange(Rk - 3, Rk), np.arange(Rk - 3, Rk)] = -0.75 * (1 - eta) / (eta / STATE_N) * (dr * e)[Rk - 3:]
        s = dict(L=L, K=np.zeros((Rk, Rk)), J=np.zeros((Rk, D)), trx=float(Rk), N=STATE_N)
    else:
        s = ref.stats(R.low_rank_batch(rng, STATE_N, D, basis))
    return ref, s


@pytest.fixture(scope="module")
def state_runs(gpu):
    """one batched update of all the cases, a second from the same inputs, and the references"""
    kf = gpu
    cases = [_state_case(D, Rk, kind, 40 + i) for i, (D, Rk, kind) in enumerate(STATE_CASES)]
    ps = Pres(kf, [(D, Rk) for D, Rk, _ in STATE_CASES])
    outs = []
    for _ in range(2):
        ps.set_state([ref for ref, _ in cases])
        ps.set_stats([s for _, s in cases])
        ps.scales()
        ps.state(1)
        outs.append((ps.read(), kf.read_f32(ps.report.ptr, (len(cases), kf.NG_REPORT))))
    refs = []
    for ref, s in cases:
        after = ref.copy()
        info = after.update_from_stats(s["L"], s["K"], s["J"], s["trx"], s["N"])
        refs.append((ref, after, info))
    return dict(outs=outs, refs=refs, ps=ps)


@pytest.mark.parametrize("i", range(len(STATE_CASES)), ids=[f"D{D}_R{Rk}_{k}" for D, Rk, k in STATE_CASES])
def test_state_against_float64(state_runs, i):
    D, Rk, kind = STATE_CASES[i]
    (got, _), rep = state_runs["outs"][0]
    before, after, info = state_runs["refs"][i]
    g = got[i]
    raw = info["raw"]
    gap = np.min(np.abs(np.diff(raw)) / np.abs(raw[:-1]))
    if kind == "equal":
        assert gap < 1e-6
    if kind == "floor":
        assert info["floored"] == 3 and np.all(np.abs(raw - info["floor"]) > 1e-3 * info["floor"])
    assert rep[i][4] == 0 and g["t"] == before.t + 1
    e_rho = abs(g["rho"] - after.rho) / after.rho
    e_d = np.max(np.abs(g["d"] - after.d) / after.d)
    Pg, Pr = g["W"].astype(F64).T @ g["W"].astype(F64), after.proj()
    e_p = np.linalg.norm(Pg - Pr) / np.linalg.norm(Pr)
    rt = g["W"].astype(F64) / np.sqrt(R.e_of(g["d"], g["rho"], D, 4.0))[:, None]
    print(f"D {D} R {Rk} {kind}: min rel gap {gap:.2e} floored {info['floored']}; rel dev rho' {e_rho:.3e} "
          f"d' {e_d:.3e} W'^T W' {e_p:.3e}; |R R^T - I|_F {np.linalg.norm(rt @ rt.T - np.eye(Rk)):.2e}")
    assert np.all(np.diff(g["d"]) <= 0)                                   # descending
    assert e_rho <= STATE_BOUND[0] and e_d <= STATE_BOUND[1] and e_p <= STATE_BOUND[2]


def test_state_is_deterministic_and_counts_steps(state_runs, gpu):
    kf = gpu
    (_, raw1), rep1 = state_runs["outs"][0]
    (_, raw2), rep2 = state_runs["outs"][1]
    for a, b in zip(raw1, raw2):
        assert np.array_equal(a.view(np.uint16 if a.dtype == np.float16 else np.uint32 if a.dtype == F32 else np.uint64),
                              b.view(np.uint16 if b.dtype == np.float16 else np.uint32 if b.dtype == F32 else np.uint64))
    assert np.array_equal(rep1.view(np.uint32), rep2.view(np.uint32))
    # a non-updating call moves nothing but t
    ps = state_runs["ps"]
    (_, (w, h, sc)) = ps.read()
    ps.state(0)
    (got, (w2, h2, sc2)) = ps.read()
    assert np.array_equal(w.view(np.uint32), w2.view(np.uint32)) and np.array_equal(h.view(np.uint16), h2.view(np.uint16))
    diff = np.flatnonzero(sc != sc2)
    assert sorted(diff) == [p.s_off + 1 for p in ps.table] and np.all(sc2[diff] == sc[diff] + 1)


def test_state_non_finite_statistic_leaves_the_state(gpu):
    kf = gpu
    cases = [_state_case(97, 8, 5, 70), _state_case(97, 8, 5, 71), _state_case(321, 32, 5, 72)]
    cases[0][1]["L"][2, 3] = np.nan
    cases[2][1]["J"][1, 5] = np.inf
    ps = Pres(kf, [(97, 8), (97, 8), (321, 32)])
    ps.set_state([ref for ref, _ in cases])
    ps.set_stats([s for _, s in cases])
    (before, _) = ps.read()
    ps.scales()
    ps.state(1)
    (got, _) = ps.read()
    rep = kf.read_f32(ps.report.ptr, (3, kf.NG_REPORT))
    assert list(rep[:, 4]) == [1.0, 0.0, 1.0]
    for i in (0, 2):
        assert np.array_equal(got[i]["W"].view(np.uint32), before[i]["W"].view(np.uint32))
        assert np.array_equal(got[i]["d"], before[i]["d"]) and got[i]["rho"] == before[i]["rho"]
        assert got[i]["t"] == before[i]["t"] + 1
    assert not np.array_equal(got[1]["W"], before[1]["W"]) and np.all(np.isfinite(got[1]["W"]))


def test_tables_are_checked(gpu):
    kf = gpu
    for D, Rk in [(97, 4), (97, 97), (400, 128)]:
        t = (kf.KfNgPre * 1)(kf.KfNgPre(D, Rk, 0, 0, 0, 0))
        assert kf.core.kf_ng_state_scratch_bytes(C.addressof(t), 1) == -1
        assert b"rank" in kf.core.kf_last_error()


# ------------------------------------------------------------------ apply kernel
APPLY_SHAPES = [(96, 32), (320, 160), (3072, 160)]
RANK_IN, RANK_OUT = 20, 80


def _clamped(rank, dim):
    return min(rank, dim // 2)


@pytest.fixture(scope="module")
def apply_runs(gpu):
    """every shape with and without the bias row, and two one-sided entries, in one call; a second
    call from the same inputs"""
    kf = gpu
    rng = np.random.default_rng(17)
    entries = [(K, N, bias, True, True) for K, N in APPLY_SHAPES for bias in (False, True)]
    entries += [(320, 160, True, True, False), (96, 40, True, False, True), (70, 50, False, True, True)]
    dims, comps, off = [], [], 12
    for K, N, bias, pin, pout in entries:
        dw = off
        off += K * N + 64
        db = -1
        if bias:
            db = off
            off += N + 64
        i_in = i_out = -1
        if pin:
            i_in = len(dims)
            dims.append((K + (1 if bias else 0), _clamped(RANK_IN, K + (1 if bias else 0))))
        if pout:
            i_out = len(dims)
            dims.append((N, _clamped(RANK_OUT, N)))
        comps.append(kf.KfNgComp(dw, db, K, N, i_in, i_out))
    n = off + 20
    ps = Pres(kf, dims)
    refs = []
    for D, Rk in dims:
        ref = R.Pre(D, Rk)
        ref.W = rng.standard_normal((Rk, D)) * (0.7 / np.sqrt(D))
        refs.append(ref)
    ps.set_state(refs)
    gam = rng.uniform(1.0, 1.6, len(dims)).astype(F32)
    rep = np.zeros((len(dims), kf.NG_REPORT), F32)
    rep[:, 0] = gam
    report = kf.upload_f32(rep)
    g0 = np.full(n, SENT32, F32)
    cov = np.zeros(n, bool)
    for c in comps:
        g0[c.dw_off:c.dw_off + c.K * c.N] = rng.standard_normal(c.K * c.N).astype(F32)
        cov[c.dw_off:c.dw_off + c.K * c.N] = True
        if c.db_off >= 0:
            g0[c.db_off:c.db_off + c.N] = rng.standard_normal(c.N).astype(F32)
            cov[c.db_off:c.db_off + c.N] = True
    table = (kf.KfNgComp * len(comps))(*comps)
    tdev = _upload_table(kf, table)
    sb = kf.core.kf_ng_apply_scratch_bytes(C.addressof(table), len(comps), C.addressof(ps.table), len(dims))
    assert sb > 0
    scratch = kf.DeviceBuffer(sb)
    outs = []
    for _ in range(2):
        g = kf.upload_f32(g0)
        kf.check(kf.core.kf_ng_apply(g.ptr, n, C.addressof(table), tdev.ptr, len(comps), *ps.args(), ps.w32.ptr,
                                     report.ptr, scratch.ptr), "kf_ng_apply")
        outs.append(kf.read_f32(g.ptr, (n,)))
    return dict(entries=entries, comps=comps, refs=refs, gam=gam, g0=g0, cov=cov, outs=outs, n=n)


def _gext(flat, c):
    g = flat[c.dw_off:c.dw_off + c.K * c.N].reshape(c.K, c.N)
    return np.vstack([g, flat[c.db_off:c.db_off + c.N][None]]) if c.db_off >= 0 else g


@pytest.mark.parametrize("i", range(9), ids=[f"{K}x{N}{'_bias' if b else ''}{'' if pi else '_noin'}{'' if po else '_noout'}"
                                             for K, N, b, pi, po in
                                             [(K, N, bias, True, True) for K, N in APPLY_SHAPES for bias in (False, True)]
                                             + [(320, 160, True, True, False), (96, 40, True, False, True),
                                                (70, 50, False, True, True)]])
def test_apply_against_float64(apply_runs, i):
    a = apply_runs
    c = a["comps"][i]
    gin = F64(a["gam"][c.pre_in]) if c.pre_in >= 0 else 1.0
    gout = F64(a["gam"][c.pre_out]) if c.pre_out >= 0 else 1.0
    ref = R.precondition_gradient(_gext(a["g0"], c), gin, gout,
                                  a["refs"][c.pre_in].proj() if c.pre_in >= 0 else None,
                                  a["refs"][c.pre_out].proj() if c.pre_out >= 0 else None)
    got = _gext(a["outs"][0], c)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"{a['entries'][i]}: rel-Frobenius {err:.3e}; moved {np.linalg.norm(got - _gext(a['g0'], c)) / np.linalg.norm(ref):.3f}")
    assert err <= 1e-5
    assert not np.array_equal(got, _gext(a["g0"], c))


def test_apply_touches_nothing_else_and_is_deterministic(apply_runs):
    a = apply_runs
    out1, out2 = a["outs"]
    assert np.array_equal(out1[~a["cov"]].view(np.uint32), a["g0"][~a["cov"]].view(np.uint32))
    assert not np.any(out1[a["cov"]] == SENT32) and np.all(np.isfinite(out1[a["cov"]]))
    assert np.array_equal(out1.view(np.uint32), out2.view(np.uint32))


def test_apply_rejects_bad_tables(gpu):
    kf = gpu
    pres = (kf.KfNgPre * 2)(kf.KfNgPre(97, 20, 0, 0, 0, 0), kf.KfNgPre(32, 16, 4000, 4000, 40, 0))
    ok = (kf.KfNgComp * 1)(kf.KfNgComp(0, 96 * 32, 96, 32, 0, 1))
    assert kf.core.kf_ng_apply_scratch_bytes(C.addressof(ok), 1, C.addressof(pres), 2) > 0
    for bad in (kf.KfNgComp(0, -1, 96, 32, 0, 1),            # no bias row: D_in would be 96
                kf.KfNgComp(0, 96 * 32, 96, 32, 1, 0),         # sides swapped
                kf.KfNgComp(0, 96 * 32, 96, 32, 0, 2)):        # no such preconditioner
        t = (kf.KfNgComp * 1)(bad)
        assert kf.core.kf_ng_apply_scratch_bytes(C.addressof(t), 1, C.addressof(pres), 2) == -1
    # a segment past the end of the buffer: refused before anything is launched
    assert kf.core.kf_ng_apply(None, 96 * 32 + 31, C.addressof(ok), None, 1, C.addressof(pres), None, 2, None, None,
                               None) == -1
    assert b"outside" in kf.core.kf_last_error()


# ------------------------------------------------------------------ trX
def _trx(kf, x, ld, nrows, T, dts, clamp, ones, edges=()):
    rows, w = x.shape
    buf = np.full((rows, ld), 60000.0, np.float16)              # what lies beyond a row's width is not read
    buf[:, :w] = x
    xb = kf.upload_fp16(buf)
    op = kf.operand(xb.ptr, ld, nrows, len(dts) * w, 0, nparts=len(dts), part_width=w, T=T,
                    tpolicy=1 if clamp else 0, dt=dts, edges=edges)
    out = kf.upload_f32(np.full(4, SENT32, F32))
    kf.check(kf.core.kf_ng_trx(C.byref(op), 1 if ones else 0, out.ptr), "kf_ng_trx")
    got = kf.read_f32(out.ptr, (4,))
    assert got[1] == nrows and np.all(got[2:] == SENT32)
    m = R.operand_rows(x.astype(F64), nrows, T, dts, clamp, edges)
    return F64(got[0]), float(np.sum(m * m)) + (nrows if ones else 0)


@pytest.mark.parametrize("ones", [False, True], ids=["plain", "ones"])
def test_trx_against_float64(gpu, ones):
    """a plain operand; the two-offset splice (-1, 0), clamped, over a sequence of 7 and one of 9
    rows (the lower edge clamps), and (0, +1) over the same (the upper edge clamps); a zero-padded
    splice whose last row reads a spare edge row; one over many workgroups"""
    kf = gpu
    rng = np.random.default_rng(23)
    cases = [("plain", dict(x=rng.standard_normal((23, 40)), ld=48, nrows=23, T=23, dts=(0,), clamp=False))]
    for T in (7, 9):
        x = rng.standard_normal((T, 24))
        cases.append((f"splice-1_T{T}", dict(x=x, ld=24, nrows=T, T=T, dts=(-1, 0), clamp=True)))
        cases.append((f"splice+1_T{T}", dict(x=x, ld=24, nrows=T, T=T, dts=(0, 1), clamp=True)))
        cases.append((f"splice-3_T{T}", dict(x=x, ld=24, nrows=T, T=T, dts=(-3, 3), clamp=True)))
    cases.append(("edge_row", dict(x=rng.standard_normal((10, 24)), ld=32, nrows=9, T=9, dts=(0, 2), clamp=False,
                                   edges=[(1, 8, 9)])))
    cases.append(("large", dict(x=rng.standard_normal((1000, 200)), ld=200, nrows=1000, T=1000, dts=(-3, 0),
                                clamp=True)))
    for name, kw in cases:
        kw["x"] = kw["x"].astype(np.float16)
        got, ref = _trx(kf, ones=ones, **kw)
        print(f"{name}: got {got:.6f} ref {ref:.6f} rel {abs(got - ref) / ref:.2e}")
        assert abs(got - ref) <= 1e-6 * ref


def test_trx_rejects_what_it_cannot_describe(gpu):
    kf = gpu
    xb = kf.upload_fp16(np.zeros((8, 16), np.float16))
    out = kf.upload_f32(np.zeros(1, F32))
    op = kf.operand(xb.ptr, 16, 16, 16, 0, T=8, hout=2, hsrc=2, hmul=1)
    assert kf.core.kf_ng_trx(C.byref(op), 0, out.ptr) == -1
    assert b"hout = 1" in kf.core.kf_last_error()


# ------------------------------------------------------------------ network level
# worst relative deviations from the float64 reference fed the same fp16 activations, seen on the
# MI355X over the 6 steps of test_network_statistics_against_float64 (gamma, rho, sum(d),
# W'^T W'); they rest on the fp16 storage of H. The bounds are 4 x these.
NET_SEEN = (6.48e-4, 4.27e-4, 1.12e-3, 9.72e-4)
NET_BOUND = tuple(4.0 * x for x in NET_SEEN)


def _flat_grad(kf, net):
    return kf.read_f32(net.grad_ptr, (net.num_params,))


def _component_tensors(net):
    """per update component: (dW tensor, db tensor or None)"""
    out = {}
    for c in net.components():
        mats = [t for t in c["tensors"] if net.params[t][0] > 1]
        vecs = [t for t in c["tensors"] if net.params[t][0] == 1]
        if len(mats) == 1 and len(vecs) <= 1:
            out[c["name"]] = (mats[0], vecs[0] if vecs else None)
    return out


def _gext_of(net, flat, dw, db):
    r, c, off = net.params[dw]
    g = flat[off:off + r * c].reshape(r, c)
    if db is not None:
        _, cb, ob = net.params[db]
        g = np.vstack([g, flat[ob:ob + cb][None]])
    return g


def _check_identity(net, G, Gh, state, stats, tag):
    """G^ = gamma_in gamma_out (I - W_in^T W_in) G (I - W_out^T W_out) for every preconditioned
    component, W and gamma as read back before the step; everything else bit-equal"""
    tensors = _component_tensors(net)
    by = {}
    flagged = [(r["name"], r["side"], r["rho"], r["sum_d"], r["gamma"]) for r in stats if r["flag"]]
    assert not flagged, (tag, flagged)
    for s, r in zip(state, stats):
        assert (s["name"], s["side"]) == (r["name"], r["side"])
        by.setdefault(s["name"], {})[s["side"]] = (s["W"].astype(F64), F64(r["gamma"]))
    touched = np.zeros(net.num_params, bool)
    for name, sides in by.items():
        dw, db = tensors[name]
        g, gh = _gext_of(net, G, dw, db), _gext_of(net, Gh, dw, db)
        win, gin = sides.get("in", (None, 1.0))
        wout, gout = sides.get("out", (None, 1.0))
        ref = R.precondition_gradient(g, gin, gout, None if win is None else win.T @ win,
                                      None if wout is None else wout.T @ wout)
        err = np.linalg.norm(gh - ref) / np.linalg.norm(ref)
        print(f"{tag} {name}: G {g.shape} ranks {None if win is None else win.shape[0]} / "
              f"{None if wout is None else wout.shape[0]} gamma {gin:.4f} {gout:.4f} rel-Frobenius {err:.2e}")
        assert err <= 1e-5, (tag, name, err)
        for t in (dw, db):
            if t is not None:
                r, c, off = net.params[t]
                touched[off:off + r * c] = True
    assert np.array_equal(Gh[~touched].view(np.uint32), G[~touched].view(np.uint32))
    for c in net.components():
        if c["name"].startswith("cnn"):
            assert c["name"] not in by
    return by


@pytest.mark.parametrize("xconfig, T, rsub", [("tiny.xconfig", 300, False), ("cnn_tdnn_17f.xconfig", 600, True)],
                         ids=["tiny_all_rows", "17f_row_subsampled"])
def test_network_identity_with_the_plain_gradient(gpu, xconfig, T, rsub):
    kf = gpu
    from kfp16 import synth
    net = kf.Network(synth.load_xconfig(xconfig), max_frames=T)
    synth.init_network(net, seed=12)
    if rsub:
        net.set_row_subsampling(3)
    feats = kf.upload_fp16(synth.make_features(T, 40, seed=4))
    net.forward(feats.ptr, T)
    assert (net.row_set()[0] > 0) == rsub
    out = net.read_activation("output")
    og = kf.upload_fp16((np.random.default_rng(8).standard_normal(out.shape) * 0.05).astype(np.float16))
    net.backward(og.ptr)
    G = _flat_grad(kf, net)
    net.set_natural_gradient(True)
    expect = {"tdnnf5.linear", "tdnnf5.affine", "prefinal-l", "prefinal-chain.affine", "prefinal-chain.linear", "output.affine"} \
        if not rsub else {"tdnnf7.linear", "tdnnf23.affine", "prefinal-l", "prefinal-chain.affine", "output.affine"}
    for step in range(6):
        state = net.natural_gradient_state() if step in (0, 5) else None
        net.forward(feats.ptr, T)
        net.backward(og.ptr)
        if state is None:
            continue
        assert all(s["t"] == step for s in state)
        by = _check_identity(net, G, _flat_grad(kf, net), state, net.natural_gradient_stats(), f"t={step}")
        assert expect <= set(by), sorted(by)
        if step == 5:   # the state has moved off its initial value and the scale is a real one
            assert all(g > 1.0 for sides in by.values() for _, g in sides.values())
    net.close()


def test_network_statistics_against_float64(gpu):
    """the output component over 6 steps on fixed inputs: its X is the activation of the layer
    below (with the ones column), its dY the output gradient the test passes"""
    kf = gpu
    from kfp16 import synth
    T = 300
    net = kf.Network(synth.load_xconfig("tiny.xconfig"), max_frames=T)
    synth.init_network(net, seed=12)
    feats = kf.upload_fp16(synth.make_features(T, 40, seed=4))
    net.forward(feats.ptr, T)
    out = net.read_activation("output")
    dy = (np.random.default_rng(8).standard_normal(out.shape) * 0.05).astype(np.float16)
    og = kf.upload_fp16(dy)
    x = net.read_activation("prefinal-chain")
    sides = {"in": np.hstack([x.astype(F64), np.ones((T, 1))]), "out": dy.astype(F64)}
    net.set_natural_gradient(True)
    idx = {s["side"]: i for i, s in enumerate(net.natural_gradient_state()) if s["name"] == "output.affine"}
    refs = {k: R.Pre(sides[k].shape[1], net.natural_gradient_state()[i]["W"].shape[0]) for k, i in idx.items()}
    assert refs["in"].R == 20 and refs["out"].R == 80
    worst = np.zeros(4)
    for step in range(6):
        net.forward(feats.ptr, T)
        net.backward(og.ptr)
        rep, state = net.natural_gradient_stats(), net.natural_gradient_state()
        for k, i in idx.items():
            ref = refs[k]
            before = ref.copy()
            _, g = ref.step(sides[k])
            r, s = rep[i], state[i]
            assert not r["flag"] and r["t"] == step and s["t"] == step + 1
            Pg, Pr = s["W"].astype(F64).T @ s["W"].astype(F64), ref.proj()
            dev = np.array([abs(r["gamma"] - g) / g, abs(r["rho"] - before.rho) / before.rho,
                            abs(r["sum_d"] - before.d.sum()) / before.d.sum(),
                            np.linalg.norm(Pg - Pr) / np.linalg.norm(Pr)])
            print(f"step {step} {k}: gamma {r['gamma']:.5f} ref {g:.5f}; rel dev gamma {dev[0]:.2e} rho {dev[1]:.2e} "
                  f"sum(d) {dev[2]:.2e} W'^T W' {dev[3]:.2e}")
            worst = np.maximum(worst, dev)
    print("worst rel dev (gamma, rho, sum(d), W'^T W'):", worst)
    assert worst[0] <= 1e-2, "fp16 H is not good enough for gamma"
    assert np.all(worst <= NET_BOUND), worst
    net.close()


def test_network_guards(gpu):
    kf = gpu
    from kfp16 import synth
    T = 150
    xcfg = synth.load_xconfig("tiny.xconfig")
    net = kf.Network(xcfg, max_frames=T)
    synth.init_network(net, seed=3)
    feats = kf.upload_fp16(synth.make_features(T, 40, seed=2))
    net.forward(feats.ptr, T)
    out = net.read_activation("output")
    og = kf.upload_fp16((np.random.default_rng(2).standard_normal(out.shape) * 0.05).astype(np.float16))
    net.backward(og.ptr)
    G = _flat_grad(kf, net)
    with pytest.raises(kf.KfError, match="natural gradient is off"):
        net.natural_gradient_stats()
    # off -> on -> off: bit-identical plain gradients again
    net.set_natural_gradient(True, rank_in=16)
    with pytest.raises(kf.KfError, match="no nnet_backward has run"):
        net.natural_gradient_stats()
    net.backward(og.ptr)
    assert not np.array_equal(_flat_grad(kf, net), G)
    assert all(s["W"].shape[0] <= 16 for s in net.natural_gradient_state() if s["side"] == "in")
    with pytest.raises(kf.KfError, match="natural gradient"):
        net.set_fp8(True)
    with pytest.raises(kf.KfError, match="natural gradient"):
        kf.check(kf.nnet.nnet_backward_n(net.h, og.ptr, 2), "nnet_backward_n")
    net.set_natural_gradient(False)
    net.backward(og.ptr)
    assert np.array_equal(_flat_grad(kf, net).view(np.uint32), G.view(np.uint32))
    assert net.natural_gradient_state() == []
    # MXFP8 mode: setting the switch is an error
    net.set_fp8(True)
    with pytest.raises(kf.KfError, match="MXFP8"):
        net.set_natural_gradient(True)
    net.set_fp8(False)
    with pytest.raises(TypeError):
        net.set_natural_gradient(True, rank=3)
    with pytest.raises(kf.KfError, match="bad options"):
        net.set_natural_gradient(True, update_period=0)
    net.close()


def test_guard_data_parallel(gpu):
    """a net bound to data parallel refuses the switch, and a net with the switch on refuses to be
    bound (nearly all of this test's time is the creation of the one-rank communicator)"""
    kf = gpu
    from kfp16 import dp, synth
    net = kf.Network(synth.load_xconfig("tiny.xconfig"), max_frames=150)
    synth.init_network(net, seed=3)
    comm = dp.Communicator(0, 1, dp.unique_id(), 0)
    net.bind_dp(comm, 1 << 20)
    with pytest.raises(kf.KfError, match="data parallel"):
        net.set_natural_gradient(True)
    net.bind_dp(None, 0)
    net.set_natural_gradient(True)
    with pytest.raises(kf.KfError, match="natural gradient"):
        net.bind_dp(comm, 1 << 20)
    comm.close()
    net.close()


def test_trainer_with_natural_gradient(gpu, tmp_path):
    """EgsTrainer with natural_gradient and kaldi_update: 8 steps on the tiny config, the objective
    stays finite and no preconditioner raises its flag"""
    kf = gpu
    import egs_writer as W
    from kfp16 import egs, synth, trainer
    rng = np.random.default_rng(31)
    exs, _ = W.make_egs(rng, 4, rows=(150, 183, 129), num_pdfs=200, fst_states=(8, 20))
    W.write_ark(tmp_path / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(tmp_path / "cegs.*.ark"), batch_size=4).next_batch()
    den = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)
    assert trainer.TrainConfig().natural_gradient is False
    tr = trainer.EgsTrainer(synth.load_xconfig("tiny.xconfig"), den, max_egs=8, max_frames=800,
                            config=trainer.TrainConfig(learning_rate=1e-3, momentum=0.9, kaldi_update=True,
                                                       max_param_change=1.0, natural_gradient=True))
    synth.init_network(tr.net)
    for step in range(8):
        tr.step(batch)
        res = tr.result()
        rep = tr.net.natural_gradient_stats()
        assert np.isfinite(res.objf) and np.isfinite(res.num_logprob) and np.isfinite(res.den_logprob)
        assert len(rep) == 24 and not any(r["flag"] for r in rep) and all(r["t"] == step for r in rep)
        assert all(np.isfinite(r["gamma"]) and r["gamma"] >= 1.0 for r in rep)
    print("gamma after 8 steps:", {(r["name"], r["side"]): round(r["gamma"], 3) for r in rep})
    w = kf.read_f32(tr.net.master_ptr, (tr.net.num_params,))
    assert np.all(np.isfinite(w))
    tr.net.close()
