"""The kernels of the ReLU statistics and self-repair (kf_ops.h kf_bn_train_stats_relu,
kf_bn_block_stats_relu, kf_relu_repair_vectors, kf_bn_train_bwd_apply_repair / _rows_repair;
DESIGN.md §31) against numpy (tests/self_repair_ref.py) and against the entries they extend.

Counts are integers and compared exactly; everything the counting entries share with the plain
ones is compared bit for bit. The apply runs test_gpu_bn_rows.py's cases and bounds: one fp16 ulp
plus the propagated bounds of a and b."""
import ctypes as C

import numpy as np
import pytest

import bn_train_ref as br
import self_repair_ref as sr
import test_gpu_bn_block as tbb
import test_gpu_bn_rows as tbr

pytestmark = pytest.mark.gpu

EPS = 1e-3
U23 = 2.0 ** -23


def _f64(kf, a):
    return kf.upload_f32(np.ascontiguousarray(a, np.float64).view(np.float32))


def _read_f64(kf, buf, n):
    return kf.read_f32(buf.ptr, (2 * n,)).view(np.float64).copy()


# ---------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------
def _run_stats(kf, entry, rb, ld, rows, dims, relu):
    """two accumulated calls -> (mean | var | scale | shift [4 x D], accumulators, relu accumulators)"""
    D = dims[-1]
    st = kf.upload_f32(np.zeros(4 * D, np.float32))
    acc = _f64(kf, np.zeros(2 + 2 * D))
    racc = _f64(kf, np.zeros(2 + D))
    p = [st.ptr + 4 * D * k for k in range(4)]
    args = [rb.ptr, ld, rows, *dims, EPS, 0.75, *p, acc.ptr, acc.ptr + 16, acc.ptr + 16 + 8 * D]
    if relu:
        args += [racc.ptr, racc.ptr + 16]
    for _ in range(2):
        kf.check(getattr(kf.core, entry)(*args), entry)
    return kf.read_f32(st.ptr, (4, D)), _read_f64(kf, acc, 2 + 2 * D), _read_f64(kf, racc, 2 + D)


@pytest.mark.parametrize("rows,D,ld", [(rows, D, D) for rows in (1, 7, 257, 1031) for D in (8, 160, 1536)] + [(257, 160, 192)])
def test_column_counts_are_exact(gpu, rows, D, ld):
    kf = gpu
    r16 = tbr._r_matrix(np.random.default_rng(rows + D), rows, D)   # column 0 all zero, column 1 all positive
    r16[:, 3] = 0
    r16[rows // 2, 3] = 0.25                                        # exactly one positive row
    rb = kf.upload_fp16(tbr._pad(r16, ld, 7))
    st1, acc1, racc = _run_stats(kf, "kf_bn_train_stats_relu", rb, ld, rows, (D,), True)
    st0, acc0, untouched = _run_stats(kf, "kf_bn_train_stats", rb, ld, rows, (D,), False)
    want = sr.relu_counts(r16)
    assert want[0] == 0 and want[1] == rows and want[3] == 1
    assert racc[0] == 2 * rows and racc[1] == 0
    assert np.array_equal(racc[2:], 2 * want)
    assert not untouched.any()
    assert np.array_equal(st1.view(np.uint32), st0.view(np.uint32))
    assert np.array_equal(acc1.view(np.uint64), acc0.view(np.uint64))


@pytest.mark.parametrize("rows,H,F", [(rows, H, F) for rows in (3, 65) for H in (10, 40) for F in (32, 64)])
def test_block_counts_are_exact(gpu, rows, H, F):
    kf = gpu
    r16 = tbb._r_matrix(np.random.default_rng(rows + H + F), rows, H, F).reshape(rows, H, F)
    r16[:, :, 3] = 0
    r16[rows // 2, H // 2, 3] = 0.25
    r16 = r16.reshape(rows, H * F)
    rb = kf.upload_fp16(r16)
    st1, acc1, racc = _run_stats(kf, "kf_bn_block_stats_relu", rb, H * F, rows, (H, F), True)
    st0, acc0, _ = _run_stats(kf, "kf_bn_block_stats", rb, H * F, rows, (H, F), False)
    want = sr.relu_counts(r16, H)
    assert want[0] == 0 and want[1] == rows * H and want[3] == 1
    assert racc[0] == 2 * rows * H
    assert np.array_equal(racc[2:], 2 * want)
    assert np.array_equal(st1.view(np.uint32), st0.view(np.uint32))
    assert np.array_equal(acc1.view(np.uint64), acc0.view(np.uint64))


def test_counting_entries_without_relu_accumulators_are_the_plain_entries(gpu):
    kf = gpu
    rows, D = 257, 160
    rb = kf.upload_fp16(tbr._r_matrix(np.random.default_rng(1), rows, D))
    st = kf.upload_f32(np.zeros(4 * D, np.float32))
    p = [st.ptr + 4 * D * k for k in range(4)]
    kf.check(kf.core.kf_bn_train_stats_relu(rb.ptr, D, rows, D, EPS, 1.0, *p, None, None, None, None, None), "stats_relu")
    a = kf.read_f32(st.ptr, (4, D))
    kf.check(kf.core.kf_bn_train_stats(rb.ptr, D, rows, D, EPS, 1.0, *p, None, None, None), "stats")
    assert np.array_equal(a.view(np.uint32), kf.read_f32(st.ptr, (4, D)).view(np.uint32))
    assert kf.core.kf_bn_train_stats_relu(rb.ptr, D, rows, D, EPS, 1.0, *p, None, None, None, st.ptr, None) == -1
    assert b"kf_bn_train_stats_relu" in kf.core.kf_last_error()
    assert kf.core.kf_bn_block_stats_relu(rb.ptr, D, rows, 2, D // 2, EPS, 1.0, *p, None, None, None, None, st.ptr) == -1
    assert b"kf_bn_block_stats_relu" in kf.core.kf_last_error()


# ---------------------------------------------------------------------------
# repair vectors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("loss_scale", [None, 1.0, 4096.0])
def test_repair_vectors(gpu, loss_scale):
    kf = gpu
    rng = np.random.default_rng(11)
    # (D, k, lower, upper, count, deriv_sum): the exact-threshold columns; count = 0; Kaldi's defaults
    d2 = rng.integers(0, 1001, 1536).astype(np.float64)
    d2[:4] = [50, 51, 950, 951]
    sites = [(8, 2.0 ** -10, 0.25, 0.75, 20.0, np.asarray([5, 6, 15, 16, 0, 20, 10, 7], np.float64)),
             (160, 1e-3, 0.05, 0.95, 0.0, rng.integers(0, 5, 160).astype(np.float64)),
             (1536, 1e-5, 0.05, 0.95, 1000.0, d2)]
    bufs, tab = [], (kf.KfRepairSite * len(sites))()
    for i, (D, k, lo, hi, count, deriv) in enumerate(sites):
        acc = _f64(kf, np.concatenate([[count, 0.0], deriv]))
        sb = kf.upload_f32(np.full(D + 8, 7.0, np.float32))
        bufs.append((acc, sb))
        tab[i] = kf.KfRepairSite(acc.ptr, acc.ptr + 16, sb.ptr, D, k, lo, hi)
    raw = bytes(tab)
    assert len(raw) == 48 * len(sites)
    tab_dev = kf.upload_f32(np.frombuffer(raw, np.float32))
    ls = kf.upload_f32(np.asarray([loss_scale, 0, 0, 0], np.float32)) if loss_scale is not None else None
    kf.check(kf.core.kf_relu_repair_vectors(C.byref(tab), tab_dev.ptr, len(sites), ls.ptr if ls else None),
             "kf_relu_repair_vectors")
    for (D, k, lo, hi, count, deriv), (_, sb) in zip(sites, bufs):
        got = kf.read_f32(sb.ptr, (D + 8,))
        want = sr.repair_vector(count, deriv, k, lo, hi, 1.0 if loss_scale is None else loss_scale)
        assert np.array_equal(got[:D], want)
        assert np.all(got[D:] == 7.0)                       # nothing past D is written
    ks = np.float32(2.0 ** -10) * np.float32(1.0 if loss_scale is None else loss_scale)
    assert kf.read_f32(bufs[0][1].ptr, (8,)).tolist() == [-ks, 0, 0, ks, -ks, ks, 0, 0]
    assert not kf.read_f32(bufs[1][1].ptr, (160,)).any()


def test_repair_vectors_argument_checks(gpu):
    kf = gpu
    buf = kf.upload_f32(np.zeros(64, np.float32))
    p = buf.ptr
    ok = kf.KfRepairSite(p, p + 16, p + 128, 8, 1e-5, 0.05, 0.95)
    for bad in (kf.KfRepairSite(p, p + 16, p + 132, 8, 1e-5, 0.05, 0.95),    # misaligned s
                kf.KfRepairSite(p, p + 16, p + 128, 12, 1e-5, 0.05, 0.95),   # D % 8
                kf.KfRepairSite(p, p + 16, p + 128, 8, -1e-5, 0.05, 0.95),
                kf.KfRepairSite(p, p + 16, p + 128, 8, 1e-5, 0.5, 0.5),
                kf.KfRepairSite(None, p + 16, p + 128, 8, 1e-5, 0.05, 0.95)):
        tab = (kf.KfRepairSite * 2)(ok, bad)
        assert kf.core.kf_relu_repair_vectors(C.byref(tab), p, 2, None) == -1
        assert b"kf_relu_repair_vectors: site 1" in kf.core.kf_last_error()
    assert kf.core.kf_relu_repair_vectors(None, p, 1, None) == -1


# ---------------------------------------------------------------------------
# apply
# ---------------------------------------------------------------------------
class _Repair(tbr._Bwd):
    """test_gpu_bn_rows.py's backward case with a repair vector drawn from {-k, 0, +k} (_case)"""

    def run_repair(self, repair="own"):
        """the statistics entry as run() calls it, then the _repair apply (rows form when srows < rows)"""
        kf, D, ld, rows = self.kf, self.D, self.ld, self.rows
        dp, sp = (self.db.ptr, self.sb_seg.ptr) if self.db else (None, None)
        mp = self.mb.ptr if self.mb else None
        a, b = self.ab.ptr, self.ab.ptr + 4 * D
        rp = self.repair if repair == "own" else repair
        kf.check(kf.core.kf_bn_train_bwd_stats_rows(self.gb.ptr, ld, self.rb.ptr, ld, rows, self.srows, D, self.scb.ptr,
                                                    self.shb.ptr, self.rms, dp, D, sp, a, b), "kf_bn_train_bwd_stats_rows")
        if self.srows < rows:
            kf.check(kf.core.kf_bn_train_bwd_apply_rows_repair(self.gb.ptr, ld, self.rb.ptr, ld, rows, self.srows, D, self.scb.ptr,
                                                               self.shb.ptr, self.rms, a, b, dp, D, sp, mp, D, self.dzb.ptr, ld,
                                                               rp), "kf_bn_train_bwd_apply_rows_repair")
        else:
            kf.check(kf.core.kf_bn_train_bwd_apply_repair(self.gb.ptr, ld, self.rb.ptr, ld, rows, D, self.scb.ptr, self.shb.ptr,
                                                          self.rms, a, b, dp, D, sp, mp, D, self.dzb.ptr, ld, rp),
                     "kf_bn_train_bwd_apply_repair")
        return kf.read_f32(self.ab.ptr, (2, D)), kf.read_fp16(self.dzb.ptr, (rows, ld))


def _case(kf, rows, srows, D, ld, with_drop, with_mask, k):
    c = _Repair.__new__(_Repair)
    tbr._Bwd.__init__(c, kf, rows, srows, D, ld, with_drop, with_mask, rows * 11 + srows + D + with_drop + 2 * with_mask)
    c.sb_seg = c.sb                      # (the base class keeps the row -> sequence map in sb)
    c.s = (np.random.default_rng(rows + D + 1).integers(-1, 2, D) * np.float32(k)).astype(np.float32)
    c.sbuf = kf.upload_f32(c.s)
    c.repair = c.sbuf.ptr
    return c


@pytest.mark.parametrize("k", [2.0 ** -10, 1e-5])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("with_drop", [False, True])
@pytest.mark.parametrize("rows,srows,D,ld", tbr.SHAPES)
def test_apply_against_float64(gpu, rows, srows, D, ld, with_drop, with_mask, k):
    c = _case(gpu, rows, srows, D, ld, with_drop, with_mask, k)
    r, g = c.r16.astype(np.float64), c.g16.astype(np.float64)
    sc, sh, rms = c.sc32.astype(np.float64), c.sh32.astype(np.float64), c.rms
    a_ref, b_ref, dz_ref = sr.repair_backward(g, r, sc, sh, rms, c.bits, c.s, srows, c.drop, c.seg if with_drop else None)
    ab1, dz1 = c.run_repair()
    dy = g * (c.drop[c.seg].astype(np.float64) if with_drop else 1.0)
    ba = U23 * np.abs(a_ref) + 1e-12 * np.abs(dy).sum(0) / srows
    bb = U23 * np.abs(b_ref) + 1e-12 * (np.abs(sc) * np.abs(dy * r).sum(0) + np.abs(sh) * np.abs(dy).sum(0)) / (rms * srows)
    yhat = (r * sc + sh) / rms
    tol = tbr._f16_ulp(dz_ref) + np.abs(sc) * (ba + np.abs(yhat) * bb) * c.bits
    got = dz1[:, :D].astype(np.float64)
    err = np.abs(got - dz_ref)
    print("dz err / tol max %.3g" % np.max(err / tol))
    assert np.all(err <= tol)
    # a masked-out element of a statistics row holds the term alone, rounded once (a subnormal at 1e-5)
    off = (c.bits[:srows] == 0)
    want_off = np.broadcast_to(c.s.astype(np.float16), (srows, D))
    assert np.array_equal(dz1[:srows, :D][off].view(np.uint16), want_off[off].view(np.uint16))
    if with_mask and k == 1e-5 and srows > 1:
        sub = np.abs(dz1[:srows, :D][off].astype(np.float64))
        assert np.any((sub > 0) & (sub < 2.0 ** -14)), "the case has no fp16-subnormal element"
    # the rows from stat_rows on: the existing _rows entry's bits
    _, dz_old = c.run("rows")
    assert np.array_equal(dz1[srows:].view(np.uint16), dz_old[srows:].view(np.uint16))
    assert np.all(dz1[:, D:] == 9)                        # nothing past D is written
    ab2, dz2 = c.run_repair()
    assert np.array_equal(ab1.view(np.uint32), ab2.view(np.uint32)) and np.array_equal(dz1.view(np.uint16), dz2.view(np.uint16))


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("with_drop", [False, True])
@pytest.mark.parametrize("rows,srows,D,ld", [(1, 1, 8, 8), (8, 5, 160, 160), (257, 250, 160, 192), (257, 257, 160, 160),
                                             (1031, 1024, 1536, 1536), (1031, 1031, 1536, 1536)])
def test_no_repair_and_zero_repair_equal_the_existing_entries(gpu, rows, srows, D, ld, with_drop, with_mask):
    kf = gpu
    c = _case(kf, rows, srows, D, ld, with_drop, with_mask, 1e-5)
    _, dz0 = c.run("rows" if srows < rows else "old")
    _, dz_null = c.run_repair(None)
    assert np.array_equal(dz_null.view(np.uint16), dz0.view(np.uint16))
    zero = kf.upload_f32(np.zeros(D, np.float32))
    _, dz_zero = c.run_repair(zero.ptr)
    assert np.array_equal(dz_zero.view(np.uint16), dz0.view(np.uint16))


def test_apply_argument_checks(gpu):
    kf = gpu
    buf = kf.upload_f32(np.zeros(512, np.float32))
    p = buf.ptr
    dz = p + 1024
    assert kf.core.kf_bn_train_bwd_apply_repair(p, 8, p, 8, 4, 8, p, p, 1.0, p, p, None, 0, None, None, 0, dz, 8, p + 4) == -1
    assert b"kf_bn_train_bwd_apply_repair: repair" in kf.core.kf_last_error()
    assert kf.core.kf_bn_train_bwd_apply_rows_repair(p, 8, p, 8, 4, 2, 8, p, p, 1.0, p, p, None, 0, None, None, 0, dz, 8, p + 4) == -1
    assert b"kf_bn_train_bwd_apply_rows_repair: repair" in kf.core.kf_last_error()
    assert kf.core.kf_bn_train_bwd_apply_repair(p, 16, p, 16, 4, 12, p, p, 1.0, p, p, None, 0, None, None, 0, dz, 16, p) == -1  # D % 8
    assert kf.core.kf_bn_train_bwd_apply_rows_repair(p, 8, p, 8, 4, 5, 8, p, p, 1.0, p, p, None, 0, None, None, 0, dz, 8, p) == -1
    assert kf.core.kf_bn_train_bwd_apply_repair(p, 8, p, 8, 4, 8, p, p, 1.0, p, p, None, 0, None, None, 0, p, 8, p + 64) == -1
    assert b"dz may not alias g or r" in kf.core.kf_last_error()                     # (the second launch reads g again)
    assert kf.core.kf_bn_train_bwd_apply_repair(p, 8, p, 8, 4, 8, p, p, 1.0, p, p, None, 0, None, None, 0, dz, 8, p + 64) == 0
    kf.sync()
