"""conv_halo_kernel (csrc/conv_halo.hip: forward and input gradient) and conv_wgrad_halo_kernel
(csrc/conv_wgrad.hip) element by element, per geometry of their dispatch, against the float64
operand rule of tests/conv_ref.py (reference semantics internal/nnet/forward.go:435-456 and
internal/gpu/backward_ops.go:162-253).

Every case
  1. asserts through kf_halo_debug_last that the halo kernel was taken, with the geometry in
     the case's id (tile, channel chunks, halo images, pitch pad, tile counts / waves, stages,
     splits, K-steps per split): a dispatch that quietly declines fails here,
  2. asserts the kf_prof_records class (4: halo forward / input gradient, 5: halo weight
     gradient, and no class 0 / 1 launch),
  3. compares every element: array_equal on the exact integer data, conv_ref's per-element bound
     on the Gaussian data (ReLU bits exact outside the bound),
  4. repeats the call and requires bit-identical output.
Source buffers carry guard frames and pad columns of 1000 (conv_ref.guarded), so a read that
should have been a zero is a gross error; every output (out, mask_out, out2, dW, bias_grad) has
a padded leading dimension and two spare rows prefilled with a sentinel that must come back
untouched. The refusals return -1 with kf_ops.h's message and leave the output untouched."""
import ctypes as C

import numpy as np
import pytest

import conv_ref as cr
from test_gpu_gemm_tiles import SENT8, SENT16, _padded16, _read_bytes, _upload_bytes, _within
from test_gpu_wgrad_tiles import SENT32, _padded32

pytestmark = pytest.mark.gpu

OFFS = cr.OFFS
FWD, DGRAD, WGRAD = cr.forward_cases(), cr.dgrad_cases(), cr.wgrad_cases()
GEMM_CLASSES = (0, 1, 4, 5)   # kf_prof classes of GEMM launches (6 is the split-K reduce)


def _src(kf, live, ld=None, guard_rows=None):
    """a guarded source on the device: (buffer, pointer to row 0)"""
    buf, off = cr.guarded(live, ld, guard_rows)
    dev = kf.upload_fp16(buf)
    return dev, dev.ptr + 2 * off


def _fused_geo(kf, geo, brow, what):
    g = kf.halo_debug_last()
    print(what, g)
    assert g["kind"] == "fused" and g["taken"] == 1, (what, g)
    got = (g["BM"], g["BN"], g["nch"], g["nbuf"], g["pad"], g["mtiles"], g["ntiles"])
    assert got == tuple(geo) and g["brow"] == brow, (what, g)
    assert g["hpos"] >= g["hpe"] > 0


def _profiled(kf, fn):
    """fn() under kf_prof_enable: (its result, the classes of the GEMM launches it made)"""
    try:
        kf.core.kf_prof_reset()
        kf.core.kf_prof_enable(1)
        res = fn()
        cls = [r["cls"] for r in kf.prof_records() if r["cls"] in GEMM_CLASSES]
    finally:
        kf.core.kf_prof_reset()
        kf.core.kf_prof_enable(0)
    return res, cls


def _f16(raw, rows, ld):
    return raw.view(np.uint16).reshape(rows, ld)


def _val(u16):
    return np.ascontiguousarray(u16).view(np.float16).astype(np.float64)


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("data", cr.DATA)
@pytest.mark.parametrize("case", FWD, ids=[c["id"] for c in FWD])
def test_forward(gpu, case, data):
    kf, c = gpu, case
    hin, fin, hout, sub, fout = c["shape"]
    d = cr.forward_inputs(c, data)
    M, N, K, T, ref = d["M"], d["N"], d["K"], c["T"], d["ref"]
    ld = hin * fin + c["ldpad"]
    xb, xp = _src(kf, d["x"], ld)
    wb, wp = _src(kf, d["W"])
    bias = kf.upload_fp16(d["bias"])
    a = kf.operand(xp, ld, M, K, 1, nparts=9, part_width=fin, T=T, hout=hout, hsrc=hin, hmul=sub, hdiv=1,
                   tpolicy=0, dt=[o[0] for o in OFFS], dh=[o[1] for o in OFFS])
    if c["tmul"] > 1:
        a.tmul, a.t0 = c["tmul"], c["t0"]
    b = kf.operand(wp, fout, K, fout, 0)
    ldo, R = N + cr.PADW, M + 2

    def launch():
        out = _upload_bytes(kf, _padded16(None, R, ldo))
        mask = _upload_bytes(kf, np.full(R * ldo // 8, SENT8, np.uint8))
        e = kf.KfEpilogue(out=out.ptr, ldo=ldo, alpha=1.0, bias=bias.ptr, relu=1, mask_out=mask.ptr)
        kf.check(kf.core.kf_gemm_fused(M, N, K, C.byref(a), C.byref(b), C.byref(e)), c["id"])
        _fused_geo(kf, c["geo"], 0, c["id"])
        kf.sync()
        res = _read_bytes(kf, out, R * ldo * 2), _read_bytes(kf, mask, R * ldo // 8)
        out.free()
        mask.free()
        return res

    raw, rawm = launch()
    got = _f16(raw, R, ldo)
    bits = cr.unpack_bits(rawm, R, ldo)
    if data == "int":
        assert np.array_equal(_val(got[:M, :N]), ref["v"]), np.argwhere(_val(got[:M, :N]) != ref["v"])[:4].tolist()
        assert np.array_equal(bits[:M, :N], ref["bits"]), "ReLU mask bits"
    else:
        _within(_val(got[:M, :N]), ref["v"], ref["tol"], "out")
        sure = ref["sure"]
        share = 1.0 - float(np.mean(sure))
        print("%s: ReLU bits exempt %.5f %%" % (c["id"], 100 * share))
        assert share <= cr.RELU_CAP
        assert np.array_equal(bits[:M, :N][sure], ref["bits"][sure]), "ReLU mask bits"
    assert (got[:M, N:] == SENT16).all() and (got[M:] == SENT16).all(), "out: padding written"
    sent = cr.unpack_bits(np.full(rawm.size, SENT8, np.uint8), R, ldo)
    assert np.array_equal(bits[:M, N:], sent[:M, N:]) and np.array_equal(bits[M:], sent[M:]), "mask_out: padding written"
    (raw2, rawm2), cls = _profiled(kf, launch)
    assert cls == [4], cls
    assert np.array_equal(raw, raw2) and np.array_equal(rawm, rawm2), "the repeated call differs"
    for buf in (xb, wb, bias):
        buf.free()


# ---------------------------------------------------------------- input gradient
def _dgrad_params():
    out = []
    for c in DGRAD:
        for bform in ("wrows", "wt") if c["kind"] != "compact" else ("wrows",):
            out.append(pytest.param(c, bform, id=c["id"] + "-" + bform))
    return out


@pytest.mark.parametrize("data", cr.DATA)
@pytest.mark.parametrize("case,bform", _dgrad_params())
def test_input_grad(gpu, case, bform, data):
    """operands as host/backward.cpp builds them (conv_dgrad_plain / _strided / _compact): the
    col2im gather of dz as A, the weights as op_wrows' shifted k-contiguous rows (BROW; the
    compact rows always) or as a transposed copy [taps * fout x fin] (dgrad_wt), out2 with
    mask_in and scale2. Each call runs once on its own sentinel-filled dx (the rows it does
    not own must stay untouched: the other residue's heights, the other frames of the compact
    form), then all calls run into one dx, which must be the first results' union bit for bit."""
    kf, c = gpu, case
    hin, fin, hout, sub, fout = c["shape"]
    d = cr.dgrad_inputs(c, data)
    P, rows = d["P"], d["rows"]
    R = rows + 2
    zb, zp = _src(kf, d["dz"])
    W = d["W"]
    wb, wp = _src(kf, W)
    sc2 = kf.upload_f32(d["scale2"])
    mk = _upload_bytes(kf, d["mask_in"])
    keep = [zb, wb, sc2, mk]
    calls = []
    for call in d["calls"]:
        taps = call["taps"]
        n = len(taps)
        a = kf.operand(zp + 2 * call["f0"] * hout * fout, hout * fout, call["M"], n * fout, 1, nparts=n,
                       part_width=fout, T=call["frames"], hout=call["rows_h"], hsrc=hout, hmul=1, hdiv=1, tpolicy=0,
                       dt=[t[1] for t in taps], dh=[t[2] for t in taps])
        if bform == "wrows":
            b = kf.operand(wp, fout, fin, n * fout, 1, nparts=n, part_width=fout, T=9 * fin, dt=[t[0] * fin for t in taps])
        else:
            wt = np.concatenate([W[t[0] * fin:(t[0] + 1) * fin].T for t in taps], 0)
            tb, tp = _src(kf, wt)
            keep.append(tb)
            b = kf.operand(tp, fin, n * fout, fin, 0)
        off, ldo2, rg, rs = 0, P, 0, 0
        if c["kind"] == "strided":
            off, ldo2 = call["pi"] * P, sub * P
        elif c["kind"] == "compact":
            off, rg, rs = (3 * call["f0"] + call["e"]) * hin * P, hin, 3 * hin
        calls.append((call, a, b, off, ldo2, rg, rs))

    def run(dx, which):
        for i in which:
            call, a, b, off, ldo2, rg, rs = calls[i]
            e = kf.KfEpilogue(alpha=1.0, out2=dx.ptr + 2 * off, ldo2=ldo2, scale2=sc2.ptr, mask_in=mk.ptr + off // 8,
                              row_group=rg, row_stride=rs)
            what = "%s call %d" % (c["id"], i)
            kf.check(kf.core.kf_gemm_fused(call["M"], fin, len(call["taps"]) * fout, C.byref(a), C.byref(b), C.byref(e)),
                     what)
            _fused_geo(kf, c["geos"][i], int(bform == "wrows"), what)
        kf.sync()
        raw = _read_bytes(kf, dx, R * P * 2)
        dx.free()
        return raw

    union = np.full((R, P), SENT16, np.uint16)
    for i, (call, *_) in enumerate(calls):
        got = _f16(run(_upload_bytes(kf, _padded16(None, R, P)), [i]), R, P)
        own = call["out_rows"]
        if data == "int":
            assert np.array_equal(_val(got[own, :fin]), d["out2"][own]), (i, "out2")
        else:
            _within(_val(got[own, :fin]), d["out2"][own], d["tol2"][own], "out2 call %d" % i)
        rest = np.ones(R, bool)
        rest[own] = False
        assert (got[rest] == SENT16).all(), "call %d wrote rows it does not own" % i
        assert (got[:, fin:] == SENT16).all(), "call %d wrote pad columns" % i
        union[own] = got[own]
    assert not (union[:rows, :fin] == SENT16).any()
    raw2, cls = _profiled(kf, lambda: run(_upload_bytes(kf, _padded16(None, R, P)), range(len(calls))))
    assert cls == [4] * len(calls), cls
    assert np.array_equal(_f16(raw2, R, P), union), "all calls into one dx differ from the single calls"
    for buf in keep:
        buf.free()


# ---------------------------------------------------------------- weight gradient
def _wgrad_geo(kf, geo, what):
    g = kf.halo_debug_last()
    print(what, g)
    assert g["kind"] == "wgrad" and g["taken"] == 1, (what, g)
    assert (g["BN"], g["waves"], g["stages"], g["splits"], g["kps"]) == tuple(geo), (what, g)
    assert 0 < g["hpw"] <= 8 and g["npieces"] <= g["hpw"] * g["waves"]


@pytest.mark.parametrize("data", cr.DATA)
@pytest.mark.parametrize("case", WGRAD, ids=[c["id"] for c in WGRAD])
def test_weight_grad(gpu, case, data):
    """dW and the bias gradient with accumulate = 0 into sentinel-filled buffers, accumulate = 1
    onto prefilled ones, a padded ldw. The time-strided case is conv_wgrad_compact's pair: the
    head frames 3c overwrite, the tail frames (t0 set, B offset past the head rows) accumulate."""
    kf, c = gpu, case
    hin, fin, hout, sub, fout = c["shape"]
    d = cr.wgrad_inputs(c, data)
    T, Mw, N = c["T"], 9 * fin, fout
    ldw = N + cr.PADW
    xb, xp = _src(kf, d["x"])
    zb, zp = _src(kf, d["dz"], guard_rows=2 * hout)
    ops = []
    for (t0, tmul, n), part in zip(cr.wgrad_calls(c), d["parts"]):
        a = kf.operand(xp, hin * fin, part["K"], Mw, 0, nparts=9, part_width=fin, T=T, hout=hout, hsrc=hin, hmul=sub,
                       hdiv=1, tpolicy=0, dt=[o[0] for o in OFFS], dh=[o[1] for o in OFFS])
        if tmul > 1:
            a.tmul, a.t0 = tmul, t0
        ops.append((a, kf.operand(zp + 2 * part["r0"] * fout, fout, part["K"], fout, 0), part))

    def run(old, first_acc):
        """the case's calls in order (the first with accumulate = first_acc, later ones 1);
        returns the raw dW / bias_grad after each call"""
        gw = _upload_bytes(kf, _padded32(d["old_w"] if old else None, Mw + 2, ldw))
        gb = _upload_bytes(kf, _padded32(d["old_b"][None] if old else None, 1, ldw)) if c["bias"] else None
        seen = []
        for i, (a, b, part) in enumerate(ops):
            what = "%s call %d" % (c["id"], i)
            kf.check(kf.core.kf_gemm_wgrad(Mw, N, part["K"], C.byref(a), C.byref(b), gw.ptr, ldw,
                                           gb.ptr if gb else None, first_acc if i == 0 else 1), what)
            _wgrad_geo(kf, c["geos"][i], what)
            kf.sync()
            seen.append((kf.read_f32(gw.ptr, (Mw + 2, ldw)), kf.read_f32(gb.ptr, (ldw,)) if gb else None))
        gw.free()
        if gb:
            gb.free()
        return seen

    def check(seen, old, what):
        w0 = d["old_w"].astype(np.float64) if old else 0.0
        b0 = d["old_b"].astype(np.float64) if old else 0.0
        wref, bref, wtol, btol = w0, b0, 0.0, 0.0
        for i, ((w, bias), (_, _, part)) in enumerate(zip(seen, ops)):
            wref, bref = wref + part["acc"], bref + part["bsum"]
            summed = old or i > 0   # the stored value is a sum rounded once more
            wtol = wtol + cr.wgrad_tol(part["K"], part["mag"], part["acc"], total=wref if summed else None)
            btol = btol + cr.wgrad_tol(part["K"], part["bmag"], part["bsum"], total=bref if summed else None)
            if data == "int":
                assert np.array_equal(w[:Mw, :N].astype(np.float64), wref), what + " dW"
            else:
                _within(w[:Mw, :N].astype(np.float64), wref, wtol, what + " dW")
            raw = w.view(np.uint32)
            assert (raw[:Mw, N:] == SENT32).all() and (raw[Mw:] == SENT32).all(), what + ": dW padding written"
            if bias is not None:
                if data == "int":
                    assert np.array_equal(bias[:N].astype(np.float64), bref), what + " db"
                else:
                    _within(bias[:N].astype(np.float64), bref, btol, what + " db")
                assert (bias.view(np.uint32)[N:] == SENT32).all(), what + ": bias_grad padding written"

    first = run(False, 0)
    check(first, False, "overwrite")
    check(run(True, 1), True, "accumulate")
    again, cls = _profiled(kf, lambda: run(False, 0))
    assert cls == [5] * len(ops), cls
    for (w, bias), (w2, bias2) in zip(first, again):
        assert np.array_equal(w.view(np.uint32), w2.view(np.uint32)), "dW differs between two runs"
        assert bias is None or np.array_equal(bias.view(np.uint32), bias2.view(np.uint32)), "db differs between two runs"
    xb.free()
    zb.free()


# ---------------------------------------------------------------- refusals
def _conv_a(kf, ptr, T, hin, fin, hout, rows, kcontig):
    return kf.operand(ptr, hin * fin, rows, 9 * fin, kcontig, nparts=9, part_width=fin, T=T, hout=hout, hsrc=hin,
                      hmul=1, hdiv=1, tpolicy=0, dt=[o[0] for o in OFFS], dh=[o[1] for o in OFFS])


def _refused(kf, rc, needle, buf, nbytes, sentinel):
    assert rc == -1
    msg = (kf.core.kf_last_error() or b"").decode()
    assert needle in msg, msg
    kf.sync()
    assert (_read_bytes(kf, buf, nbytes) == sentinel).all(), "a refused call wrote its output"


def _refusal_setup(kf, hin, fin, fout, T, out_elems, esize):
    rng = np.random.default_rng(5)
    xb, xp = _src(kf, cr.h16(rng.integers(-2, 3, (T, hin * fin))))
    wb, wp = _src(kf, cr.h16(rng.integers(-1, 2, (max(9 * fin, T * hin), max(fout, fin)))))
    out = _upload_bytes(kf, np.full(out_elems * esize, SENT8, np.uint8))
    kf.core.kf_clear_error()
    return xb, xp, wb, wp, out


def test_refuses_tmul_on_declined_forward(gpu):
    """32 input filters: the halo kernel declines, and the im2col GEMM has no time-strided rows"""
    kf = gpu
    hin, fin, fout, T, nc = 10, 32, 64, 13, 5
    M = nc * hin
    xb, xp, wb, wp, out = _refusal_setup(kf, hin, fin, fout, T, M * fout, 2)
    a = _conv_a(kf, xp, T, hin, fin, hin, M, 1)
    a.tmul = 3
    b = kf.operand(wp, max(fout, fin), 9 * fin, fout, 0)
    e = kf.KfEpilogue(out=out.ptr, ldo=fout, alpha=1.0)
    rc = kf.core.kf_gemm_fused(M, fout, 9 * fin, C.byref(a), C.byref(b), C.byref(e))
    assert kf.halo_debug_last()["taken"] == 0
    _refused(kf, rc, "need a conv on the halo kernel", out, M * fout * 2, SENT8)


def test_refuses_tmul_on_declined_weight_grad(gpu):
    """(10,256,10,1,64) with tmul = 3: 36 halo pieces on 4 waves, and N % 128 != 0 rules out 8"""
    kf = gpu
    hin, fin, fout, T, nc = 10, 256, 64, 13, 5
    K = nc * hin
    xb, xp, wb, wp, out = _refusal_setup(kf, hin, fin, fout, T, 9 * fin * fout, 4)
    a = _conv_a(kf, xp, T, hin, fin, hin, K, 0)
    a.tmul = 3
    b = kf.operand(wp, 256, K, fout, 0)
    rc = kf.core.kf_gemm_wgrad(9 * fin, fout, K, C.byref(a), C.byref(b), out.ptr, fout, None, 0)
    g = kf.halo_debug_last()
    assert g["kind"] == "wgrad" and g["taken"] == 0, g
    _refused(kf, rc, "need a 3x3 conv on the halo kernel", out, 9 * fin * fout * 4, SENT8)


@pytest.mark.parametrize("why", ["plainB", "stride<group"])
def test_refuses_row_group(gpu, why):
    """grouped output rows: only with op_wrows' B (the BROW kernels), and row_stride >= row_group"""
    kf = gpu
    hin, fin, fout, T = 10, 64, 64, 4
    M = T * hin
    xb, xp, wb, wp, out = _refusal_setup(kf, hin, fout, fin, T, 3 * M * fin, 2)
    taps = cr.dgrad_compact_taps(OFFS, 0)
    a = kf.operand(xp, hin * fout, M, 3 * fout, 1, nparts=3, part_width=fout, T=T, hout=hin, hsrc=hin, hmul=1, hdiv=1,
                   tpolicy=0, dt=[t[1] for t in taps], dh=[t[2] for t in taps])
    if why == "plainB":
        b = kf.operand(wp, 64, 3 * fout, fin, 0)
        stride, needle = 3 * hin, "need a conv on the halo kernel"
    else:
        b = kf.operand(wp, 64, fin, 3 * fout, 1, nparts=3, part_width=fout, T=9 * fin, dt=[t[0] * fin for t in taps])
        stride, needle = hin - 1, "row_stride >= row_group"
    e = kf.KfEpilogue(alpha=1.0, out2=out.ptr, ldo2=fin, row_group=hin, row_stride=stride)
    rc = kf.core.kf_gemm_fused(M, fin, 3 * fout, C.byref(a), C.byref(b), C.byref(e))
    _refused(kf, rc, needle, out, 3 * M * fin * 2, SENT8)


@pytest.mark.parametrize("entry", ["fused", "wgrad"])
def test_refuses_tmul_on_operand_b(gpu, entry):
    kf = gpu
    hin, fin, fout, T = 10, 64, 64, 4
    M = T * hin
    xb, xp, wb, wp, out = _refusal_setup(kf, hin, fin, fout, T, 9 * fin * fout, 4)
    if entry == "fused":
        a = _conv_a(kf, xp, T, hin, fin, hin, M, 1)
        b = kf.operand(wp, 64, 9 * fin, fout, 0)
        b.tmul = 3
        e = kf.KfEpilogue(out=out.ptr, ldo=fout, alpha=1.0)
        rc = kf.core.kf_gemm_fused(M, fout, 9 * fin, C.byref(a), C.byref(b), C.byref(e))
        needle = "operand B: time-strided rows"
    else:
        a = _conv_a(kf, xp, T, hin, fin, hin, M, 0)
        b = kf.operand(wp, 64, M, fout, 0)
        b.t0 = 1
        rc = kf.core.kf_gemm_wgrad(9 * fin, fout, M, C.byref(a), C.byref(b), out.ptr, fout, None, 0)
        needle = "only on the conv im2col operand A"
    _refused(kf, rc, needle, out, 9 * fin * fout * 4, SENT8)
