"""The dynamic loss scale's kernels on the GPU (kf_ops.h kf_loss_scale_*, csrc/loss_scale.hip,
DESIGN.md §30): the check pass over segment tables, the state machine against
tests/loss_scale_ref.py, the exactness of the unscale (a power-of-two scale leaves the update
bit-identical to the plain one on the unscaled gradient) and the skipped step.

Every comparison here is exact: the check's decision is a boolean, the state is small integers and
powers of two, and g * 2^k * 2^-k is g for |g| in [1e-6, 1] and k <= 16 (no product leaves
fp32's normal range)."""
import ctypes as C

import numpy as np
import pytest

from loss_scale_ref import LossScaleRef, overflow_of

pytestmark = pytest.mark.gpu

F32 = np.float32
CHUNK = 4096


def _bits(a):
    return a.view(np.uint32) if a.dtype == F32 else a.view(np.uint16)


def _tables(kf, comps):
    """device tables of kf_ops.h from [(segments [(b, e)], max_change, l2, lr_factor)]"""
    assert kf.UPD_CHUNK == CHUNK
    segs, cs, wg = [], [], 0
    for ci, (ss, mc, l2, lrf) in enumerate(comps):
        first = wg
        for b, e in ss:
            segs.append((b, e, ci, wg))
            wg += -(-(e - b) // CHUNK)
        cs.append((mc, l2, lrf, first, wg - first))
    sa = (kf.KfUpdSegment * len(segs))(*[kf.KfUpdSegment(*s) for s in segs])
    ca = (kf.KfUpdComp * len(cs))(*[kf.KfUpdComp(*c) for c in cs])

    def up(arr):
        buf = kf.DeviceBuffer(C.sizeof(arr))
        kf.check(kf.core.bridge_transfer_int32(buf.ptr, C.addressof(arr), C.sizeof(arr) // 4), "tables")
        return buf
    return up(sa), len(segs), up(ca), len(cs)


class Scaler:
    """a device state block and the check pass over one segment table"""

    def __init__(self, kf, n, comps, **opts):
        self.kf, self.n = kf, n
        self.segs, self.nseg, self.cbuf, self.ncomp = _tables(kf, comps)
        assert kf.core.kf_loss_scale_state_bytes() >= 28
        self.state = kf.DeviceBuffer(kf.core.kf_loss_scale_state_bytes())
        sb = kf.core.kf_loss_scale_scratch_bytes(n, self.nseg)
        assert sb == (n // CHUNK + self.nseg) * 4
        self.flags = kf.DeviceBuffer(sb)
        o = kf.KfLossScaleOpts()
        kf.core.kf_loss_scale_default_opts(C.byref(o))
        assert (o.init_scale, o.growth, o.backoff, o.growth_interval, o.min_scale, o.max_scale) == \
            (65536.0, 2.0, 0.5, 2000, 1.0, 65536.0)
        for k, v in opts.items():
            setattr(o, k, v)
        kf.check(kf.core.kf_loss_scale_init(self.state.ptr, C.byref(o)), "kf_loss_scale_init")

    def check(self, g_ptr):
        kf = self.kf
        kf.check(kf.core.kf_loss_scale_check(self.state.ptr, g_ptr, self.n, self.segs.ptr, self.nseg, self.ncomp,
                                             self.flags.ptr), "kf_loss_scale_check")

    def read(self):
        kf = self.kf
        s, since, steps, skipped, last = C.c_float(), C.c_int(), C.c_longlong(), C.c_longlong(), C.c_int()
        kf.check(kf.core.kf_loss_scale_read(self.state.ptr, C.byref(s), C.byref(since), C.byref(steps),
                                            C.byref(skipped), C.byref(last)), "kf_loss_scale_read")
        return dict(scale=s.value, since=since.value, steps=steps.value, skipped=skipped.value,
                    last_overflow=bool(last.value))


# ------------------------------------------------------------------ the check pass
def _base(n, seed):
    """finite everywhere, with the extremes of the finite range in it"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n).astype(F32)
    k = min(n, 8)
    g[rng.choice(n, k, replace=False)] = np.array([3e38, -3e38, 1e-45, -1e-45, 1e-39, -1e-39, 0.0, -0.0], F32)[:k]
    return g


def _positions(segs, n):
    """(index, inside a segment) of the places a non-finite value is planted at"""
    pos = set()
    for b, e in segs:
        pos |= {b, e - 1}                                   # first and last element
        for c in range(b + CHUNK, e, CHUNK):                # either side of a chunk boundary
            pos |= {c - 1, c}
        a0 = min(-(-b // 4) * 4, e)                         # the first chunk's scalar head [b, a0)
        pos |= set(range(b, a0))
        last = b + (e - 1 - b) // CHUNK * CHUNK             # the last chunk's scalar tail
        la0 = min(-(-last // 4) * 4, e)
        pos |= set(range(la0 + (e - la0) // 4 * 4, e))
    inside = np.zeros(n, bool)
    for b, e in segs:
        inside[b:e] = True
    gaps = np.flatnonzero(~inside)
    pos |= {int(gaps[0]), int(gaps[-1]), int(gaps[len(gaps) // 2])}
    for b, e in segs:                                       # the elements just outside a segment
        pos |= {i for i in (b - 1, e) if 0 <= i < n and not inside[i]}
    return sorted(pos), inside


THREE = [(3, 4102), (4110, 4117), (5001, 13501)]  # unaligned begins and ends, gaps, 2 and 3 chunks, one of 7 elements
TABLES = {"one-1": ([(0, 1)], 8), "one-4095": ([(0, 4095)], 4104), "one-4096": ([(0, 4096)], 4104),
          "one-4097": ([(0, 4097)], 4104), "three": (THREE, 13600)}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_check_pass_decision(gpu, name):
    kf = gpu
    segs, n = TABLES[name]
    sc = Scaler(kf, n, [([s], 0.0, 0.0, 1.0) for s in segs], init_scale=1024.0)
    base = _base(n, 5)
    gbuf = kf.upload_f32(base)
    sc.check(gbuf.ptr)
    st = sc.read()
    assert not overflow_of(base, segs)
    assert not st["last_overflow"] and st["skipped"] == 0 and st["steps"] == 1, "±3e38 and subnormals are finite"
    pos, inside = _positions(segs, n)
    assert inside[pos].any() and (~inside[pos]).any()
    steps, skipped, n_gap = 1, 0, 0
    for i in pos:
        for bad in (np.inf, -np.inf, np.nan):
            g = base.copy()
            g[i] = bad
            kf.check(kf.core.bridge_transfer_float32(gbuf.ptr, g.ctypes.data, n), "upload")
            sc.check(gbuf.ptr)
            st = sc.read()
            want = overflow_of(g, segs)
            assert want == bool(inside[i])
            steps, skipped, n_gap = steps + 1, skipped + int(want), n_gap + int(not want)
            assert st["last_overflow"] == want, f"{name}: {bad} at {i} ({'segment' if inside[i] else 'gap'})"
            assert (st["steps"], st["skipped"]) == (steps, skipped)
    assert n_gap >= 9 and skipped >= 3


def test_check_pass_many_bad_elements_and_all_gaps_bad(gpu):
    """every gap element non-finite: clean; every segment element non-finite: one overflow"""
    kf = gpu
    segs, n = TABLES["three"]
    sc = Scaler(kf, n, [([s], 0.0, 0.0, 1.0) for s in segs])
    _, inside = _positions(segs, n)
    g = _base(n, 6)
    g[~inside] = np.nan
    sc.check(kf.upload_f32(g).ptr)
    assert not sc.read()["last_overflow"]
    g = _base(n, 6)
    g[inside] = np.inf
    sc.check(kf.upload_f32(g).ptr)
    st = sc.read()
    assert st["last_overflow"] and st["skipped"] == 1 and st["scale"] == 32768.0


# ------------------------------------------------------------------ the state machine
def test_state_machine_follows_the_rule(gpu):
    """12 steps from scale 4 in [1, 16] with growth_interval 3: six clean steps reach the ceiling 16,
    five overflows reach the floor 1 and are held there, one clean step after"""
    kf = gpu
    segs, n = TABLES["three"]
    opts = dict(init_scale=4.0, growth_interval=3, min_scale=1.0, max_scale=16.0)
    sc = Scaler(kf, n, [([s], 0.0, 0.0, 1.0) for s in segs], **opts)
    ref = LossScaleRef(**opts)
    assert sc.read() == ref.stats()
    clean = _base(n, 7)
    bad = clean.copy()
    bad[THREE[2][0] + CHUNK] = np.inf
    gc, gb = kf.upload_f32(clean), kf.upload_f32(bad)
    pattern = [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0]
    scales = []
    for ov in pattern:
        sc.check((gb if ov else gc).ptr)
        ref.update(bool(ov))
        st = sc.read()
        assert st == ref.stats()
        scales.append(st["scale"])
    assert scales == [4, 4, 8, 8, 8, 16, 8, 4, 2, 1, 1, 1] and st["skipped"] == 5 and st["steps"] == 12
    # set_scale: clamped, the clean-step count starts again
    kf.check(kf.core.kf_loss_scale_set_scale(sc.state.ptr, 1e9), "set_scale")
    ref.set_scale(1e9)
    assert sc.read() == ref.stats() and sc.read()["scale"] == 16.0


def test_bad_options_are_refused(gpu):
    kf = gpu
    state = kf.DeviceBuffer(kf.core.kf_loss_scale_state_bytes())
    for field, v in (("init_scale", 0.0), ("growth", 0.5), ("backoff", 0.0), ("backoff", 1.5), ("growth_interval", 0),
                     ("min_scale", 0.0), ("max_scale", 0.5), ("init_scale", float("nan"))):
        o = kf.KfLossScaleOpts()
        kf.core.kf_loss_scale_default_opts(C.byref(o))
        setattr(o, field, v)
        assert kf.core.kf_loss_scale_init(state.ptr, C.byref(o)) == -1, (field, v)
        assert b"kf_loss_scale_init" in kf.core.kf_last_error()
    assert kf.core.kf_loss_scale_init(None, None) == -1


# ------------------------------------------------------------------ the scaled updates
N_FLAT = 60016
SEGS = [[(5, 9000)], [(9011, 13000), (13050, 30001)], [(30016, 59999)]]
LR, MOM, L2S = 1e-2, 0.9, 8.0


@pytest.fixture(scope="module")
def flat():
    rng = np.random.default_rng(77)
    n = N_FLAT
    # |g| log-uniform in [1e-6, 1]
    g = (10.0 ** rng.uniform(-6, 0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    assert np.all(np.abs(g) >= 1e-6) and np.all(np.abs(g) <= 1)
    w = (rng.standard_normal(n) * 0.1).astype(F32)
    v = (rng.standard_normal(n) * 0.05).astype(F32)
    # max-changes at half the float64 norms of the unlimited step, the global limit at half of what is left
    opts = [(0.01, 1.0), (0.0, 0.5), (0.005, 0.333)]
    norms = []
    for ss, (l2, lrf) in zip(SEGS, opts):
        idx = np.concatenate([np.arange(b, e) for b, e in ss])
        vv = MOM * v[idx].astype(np.float64) + g[idx] + L2S * l2 * w[idx]
        norms.append(np.sqrt(np.sum((LR * lrf * vv) ** 2)))
    mc = [0.5 * norms[0], 0.5 * norms[1], 0.0]
    mpc = 0.5 * np.sqrt((0.5 * norms[0]) ** 2 + (0.5 * norms[1]) ** 2 + norms[2] ** 2)
    comps = [(ss, F32(m), F32(l2), F32(lrf)) for ss, m, (l2, lrf) in zip(SEGS, mc, opts)]
    for a in (w, g, v):
        a.setflags(write=False)
    return dict(w=w, g=g, v=v, comps=comps, mpc=float(mpc))


class Buffers:
    def __init__(self, kf, fl, g):
        self.kf = kf
        self.w, self.v, self.g = kf.upload_f32(fl["w"]), kf.upload_f32(fl["v"]), kf.upload_f32(g)
        self.h = kf.upload_fp16(fl["w"].astype(np.float16))
        self.stats = None

    def read(self):
        kf, n = self.kf, N_FLAT
        out = [kf.read_f32(self.w.ptr, (n,)), kf.read_fp16(self.h.ptr, (n,)), kf.read_f32(self.v.ptr, (n,))]
        if self.stats is not None:
            out.append(kf.read_f32(self.stats.ptr, (2 * 3 + 2,)))
        return out


def _update(kf, fl, g, sc=None, scaled_entry=False):
    """one kf_update_maxchange on fresh buffers; with sc: check, then the scaled call"""
    b = Buffers(kf, fl, g)
    tab = sc if sc is not None else Scaler(kf, N_FLAT, fl["comps"])
    scratch = kf.DeviceBuffer(kf.core.kf_update_scratch_bytes(N_FLAT, tab.nseg, tab.ncomp))
    b.stats = kf.upload_f32(np.full(8, -3.0, F32))
    args = (b.w.ptr, b.h.ptr, b.g.ptr, b.v.ptr, N_FLAT, tab.segs.ptr, tab.nseg, tab.cbuf.ptr, tab.ncomp, LR, MOM,
            fl["mpc"], L2S, scratch.ptr, b.stats.ptr)
    if sc is not None:
        sc.check(b.g.ptr)
        kf.check(kf.core.kf_update_maxchange_scaled(*args, sc.state.ptr), "kf_update_maxchange_scaled")
    elif scaled_entry:
        kf.check(kf.core.kf_update_maxchange_scaled(*args, None), "kf_update_maxchange_scaled")
    else:
        kf.check(kf.core.kf_update_maxchange(*args), "kf_update_maxchange")
    return b.read()


def _sgd(kf, fl, g, sc=None):
    b = Buffers(kf, fl, g)
    args = (b.w.ptr, b.h.ptr, b.g.ptr, b.v.ptr, LR, MOM, N_FLAT - 1)   # (an n that is no multiple of 4)
    if sc is not None:
        sc.check(b.g.ptr)
        kf.check(kf.core.kf_sgd_flat_scaled(*args, sc.state.ptr), "kf_sgd_flat_scaled")
    else:
        kf.check(kf.core.kf_sgd_flat(*args), "kf_sgd_flat")
    return b.read()


@pytest.fixture(scope="module")
def plain(gpu, flat):
    """today's calls on the unscaled gradient, computed once"""
    upd = _update(gpu, flat, flat["g"])
    stats = upd[3]
    assert stats[3] < 1 and stats[4] < 1 and stats[5] == 1 and stats[7] < 1, "max-change and the global limit both bite"
    sgd = _sgd(gpu, flat, flat["g"])
    for a in upd + sgd:
        a.setflags(write=False)
    return dict(upd=upd, sgd=sgd)


def _same(got, want, what):
    assert len(got) == len(want)
    for name, a, b in zip(("w32", "w16", "v", "stats"), got, want):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{what}: {name}")


@pytest.mark.parametrize("k", [0, 7, 16])
def test_unscale_is_exact(gpu, flat, plain, k):
    kf, s = gpu, F32(2.0 ** k)
    gs = flat["g"] * s
    assert np.array_equal((gs * (F32(1) / s)), flat["g"])
    sc = Scaler(kf, N_FLAT, flat["comps"], init_scale=float(s), growth_interval=1000)
    _same(_update(kf, flat, gs, sc), plain["upd"], f"update, scale 2^{k}")
    _same(_sgd(kf, flat, gs, sc), plain["sgd"], f"sgd, scale 2^{k}")
    st = sc.read()
    assert (st["scale"], st["since"], st["steps"], st["skipped"], st["last_overflow"]) == (float(s), 2, 2, 0, False)


def test_null_state_is_the_plain_call(gpu, flat, plain):
    _same(_update(gpu, flat, flat["g"], scaled_entry=True), plain["upd"], "state NULL")


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_overflow_skips_the_step(gpu, flat, plain, bad):
    """one non-finite element: w32, w16 and v keep their bits, the report is all zero, the scale halves"""
    kf = gpu
    gs = flat["g"] * F32(128.0)
    gs[SEGS[1][1][0] + CHUNK + 1] = bad
    sc = Scaler(kf, N_FLAT, flat["comps"], init_scale=128.0)
    b0 = Buffers(kf, flat, gs).read()
    w32, w16, v, stats = _update(kf, flat, gs, sc)
    _same([w32, w16, v], b0, "skipped update")
    assert np.array_equal(stats, np.zeros(8, F32)), stats
    st = sc.read()
    assert (st["scale"], st["since"], st["steps"], st["skipped"], st["last_overflow"]) == (64.0, 0, 1, 1, True)
    _same(_sgd(kf, flat, gs, sc), b0, "skipped sgd")
    st = sc.read()
    assert (st["scale"], st["steps"], st["skipped"]) == (32.0, 2, 2)
    # the next clean gradient was made with scale 32: it is unscaled by 1/32, not by the state's new scale
    g32 = flat["g"] * F32(32.0)
    _same(_update(kf, flat, g32, sc), plain["upd"], "the step after the skips")
    assert sc.read()["skipped"] == 2 and sc.read()["since"] == 1
