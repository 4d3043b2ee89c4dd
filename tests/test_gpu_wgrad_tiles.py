"""kf_gemm_wgrad / kf_gemm_wgrad_scaled on every tile of their dispatch (csrc/gemm_wgrad.hip
wgrad_impl), at a single split and at the default split-K target, against float64
(tests/gemm_ref.py; reference semantics internal/gpu/backward_ops.go:162-253: dW = A^T B,
db = column sums of B).

Per case: overwrite and accumulate onto prefilled dW / bias_grad, a padded ldw whose pad
columns and two spare rows must come back untouched, bias_grad present and NULL, and the
column-scaled form. Every element of dW and db is checked. The first call is repeated under
kf_prof_enable: the record names the tile, and the repeat is bit-identical (kf_ops.h: slab
reduction in split order, no atomics). Operands beyond the plain ones: the two-part splice
whose parts' tiles are paired per XCD (WgradArgs::pair_ps), the general im2col operand on a
conv the halo kernel declines, and a masked B with a plain and a two-part A."""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as gr

pytestmark = pytest.mark.gpu

SENT32 = 0x7FC12345   # an fp32 NaN pattern
CASES = gr.wgrad_cases()
# (accumulate, bias_grad, col_scale); the first one is the repeated, profiled call
VARIANTS = [(0, True, False), (1, False, False), (1, True, True), (0, False, True)]


def _upload_bytes(kf, arr):
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    assert a.size % 4 == 0
    buf = kf.DeviceBuffer(a.size)
    kf.check(kf.core.bridge_transfer_int32(buf.ptr, a.ctypes.data, a.size // 4), "upload")
    return buf


def _padded32(live, rows, ld):
    host = np.full((rows, ld), SENT32, np.uint32)
    if live is not None:
        host[:live.shape[0], :live.shape[1]] = np.ascontiguousarray(live, np.float32).view(np.uint32)
    return host


def _operands(kf, c, d):
    M, N, T = c["M"], c["N"], c["T"]
    keep = [kf.upload_fp16(d["x"]), kf.upload_fp16(d["Bs"])]
    if c["a"] == "plain":
        a = kf.operand(keep[0].ptr, M, T, M, 0)
    elif c["a"] == "im2col":
        g = gr.IM2COL
        a = kf.operand(keep[0].ptr, g["hin"] * g["fin"], T, M, 0, nparts=9, part_width=g["fin"], T=g["frames"],
                       hout=g["hout"], hsrc=g["hin"], hmul=g["sub"], hdiv=1, tpolicy=0,
                       dt=[o[0] for o in g["offs"]], dh=[o[1] for o in g["offs"]])
    else:
        a = kf.operand(keep[0].ptr, c["part"], T, M, 0, nparts=2, part_width=c["part"],
                       tpolicy=gr.KF_CLAMP if c["a"] == "clamp" else gr.KF_ZERO, dt=(-gr.S, 0))
    mk = {}
    if c["maskb"]:
        keep.append(_upload_bytes(kf, d["bmask"]))
        mk = dict(mask=keep[-1].ptr, mask_rows=T)
    b = kf.operand(keep[1].ptr, N, T, N, 0, **mk)
    return a, b, keep


def _run(kf, c, d, a, b, dcs, accumulate, with_bias, scaled):
    M, N, T = c["M"], c["N"], c["T"]
    ldw = N + 8
    gw = _upload_bytes(kf, _padded32(d["old_w"] if accumulate else None, M + 2, ldw))
    gb = _upload_bytes(kf, _padded32(d["old_b"][None] if accumulate else None, 1, ldw)) if with_bias else None
    gbp = gb.ptr if gb else None
    if scaled:
        rc = kf.core.kf_gemm_wgrad_scaled(M, N, T, C.byref(a), C.byref(b), gw.ptr, ldw, gbp, accumulate, dcs.ptr)
    else:
        rc = kf.core.kf_gemm_wgrad(M, N, T, C.byref(a), C.byref(b), gw.ptr, ldw, gbp, accumulate)
    kf.check(rc, c["id"])
    kf.sync()
    w = kf.read_f32(gw.ptr, (M + 2, ldw))
    bias = kf.read_f32(gb.ptr, (ldw,)) if gb else None
    return w, bias


def _within(got, ref, tol, what):
    bad = ~(np.abs(got - ref) <= tol)   # a NaN fails
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(),
                           float(np.nanmax(np.abs(got - ref) - tol)))


def _check(c, d, w, bias, accumulate, scaled, what):
    M, N, T = c["M"], c["N"], c["T"]
    cs = d["col_scale"] if scaled else None
    cs64 = d["col_scale"].astype(np.float64) if scaled else 1.0
    ref = d["acc"] * cs64 + (d["old_w"].astype(np.float64) if accumulate else 0.0)
    _within(w[:M, :N].astype(np.float64), ref, gr.wgrad_tol(T, d["mag"], d["acc"], cs, ref if accumulate else None),
            what + " dW")
    raw = w.view(np.uint32)
    assert (raw[:M, N:] == SENT32).all(), what + ": dW pad columns written"
    assert (raw[M:] == SENT32).all(), what + ": dW rows past M written"
    if bias is not None:
        bref = d["bsum"] * cs64 + (d["old_b"].astype(np.float64) if accumulate else 0.0)
        _within(bias[:N].astype(np.float64), bref,
                gr.wgrad_tol(T, d["bmag"], d["bsum"], cs, bref if accumulate else None), what + " db")
        assert (bias.view(np.uint32)[N:] == SENT32).all(), what + ": bias_grad padding written"


@pytest.mark.parametrize("target", [1, 512], ids=["single-split", "default-target"])
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_wgrad_tile(gpu, case, target):
    kf = gpu
    c = case
    d = gr.wgrad_inputs(c)
    a, b, keep = _operands(kf, c, d)
    dcs = kf.upload_f32(d["col_scale"])
    old_target = kf.core.kf_gemm_wgrad_target(target)
    try:
        first = None
        for accumulate, with_bias, scaled in VARIANTS:
            what = "%s acc=%d bias=%d scaled=%d" % (c["id"], accumulate, with_bias, scaled)
            w, bias = _run(kf, c, d, a, b, dcs, accumulate, with_bias, scaled)
            _check(c, d, w, bias, accumulate, scaled, what)
            if first is None:
                first = (w, bias)
        # the first call once more, profiled: its tile, and the same bits (deterministic reduce)
        try:
            kf.core.kf_prof_reset()
            kf.core.kf_prof_enable(1)
            w2, bias2 = _run(kf, c, d, a, b, dcs, *VARIANTS[0])
            tiles = [r["tile"] for r in kf.prof_records() if r["cls"] == 1]
        finally:
            kf.core.kf_prof_reset()
            kf.core.kf_prof_enable(0)
    finally:
        kf.core.kf_gemm_wgrad_target(old_target)
    assert tiles == [c["tile"][0] * 10000 + c["tile"][1]], (tiles, c["tile"])
    assert np.array_equal(first[0].view(np.uint32), w2.view(np.uint32)), "dW differs between two runs"
    assert np.array_equal(first[1].view(np.uint32), bias2.view(np.uint32)), "db differs between two runs"
    for buf in keep + [dcs]:
        buf.free()


@pytest.mark.parametrize("with_bias", [False, True], ids=["dW", "dW+db"])
def test_wgrad_reduce_timed_and_untimed(gpu, with_bias):
    """The slab reduce runs one of two kernels (dW alone, or dW and the bias columns in one
    launch), each on the plain or the timed launch path. On the smallest case, at the default
    target (four splits): a profiled call leaves exactly one wgrad record (class 1) and one
    reduce record (class 6), and its dW and db carry the bits of the unprofiled call."""
    kf = gpu
    c = min(CASES, key=lambda k: k["M"] * k["N"])
    d = gr.wgrad_inputs(c)
    a, b, keep = _operands(kf, c, d)
    assert c["T"] >= 2 * 4 * 64   # one tile, at least 4 K-steps per split: at least two splits
    old_target = kf.core.kf_gemm_wgrad_target(512)   # the default
    try:
        w, bias = _run(kf, c, d, a, b, None, 0, with_bias, False)
        _check(c, d, w, bias, 0, False, c["id"])
        try:
            kf.core.kf_prof_reset()
            kf.core.kf_prof_enable(1)
            w2, bias2 = _run(kf, c, d, a, b, None, 0, with_bias, False)
            classes = [r["cls"] for r in kf.prof_records()]
        finally:
            kf.core.kf_prof_reset()
            kf.core.kf_prof_enable(0)
    finally:
        kf.core.kf_gemm_wgrad_target(old_target)
    assert classes.count(1) == 1 and classes.count(6) == 1, classes
    assert np.array_equal(w.view(np.uint32), w2.view(np.uint32)), "dW differs under profiling"
    if with_bias:
        assert np.array_equal(bias.view(np.uint32), bias2.view(np.uint32)), "db differs under profiling"
    for buf in keep:
        buf.free()


def test_wgrad_target_query_and_restore(gpu):
    """kf_gemm_wgrad_target returns the previous value; a value <= 0 only queries"""
    kf = gpu
    cur = kf.core.kf_gemm_wgrad_target(0)
    assert cur > 0
    try:
        assert kf.core.kf_gemm_wgrad_target(7) == cur
        assert kf.core.kf_gemm_wgrad_target(-1) == 7
        assert kf.core.kf_gemm_wgrad_target(0) == 7
    finally:
        assert kf.core.kf_gemm_wgrad_target(cur) == 7
    assert kf.core.kf_gemm_wgrad_target(0) == cur
