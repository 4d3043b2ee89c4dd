"""kf_gemm_fused on every tile of its dispatch (csrc/gemm_fused.hip fused_impl), each with ragged
tails, padded leading dimensions and every epilogue term, against the float64 rule of
tests/gemm_ref.py (include/kf_ops.h KfEpilogue; reference semantics cpp/cuda/ops.cu:381-392 and
internal/nnet/forward.go:589-695 for the terms the epilogue folds in).

fused_epilogue is a different instantiation per tile (items per lane, the residual register
ring, the swizzled staging, the MXFP8 copy), so each case proves the tile it ran on: the call
is repeated under kf_prof_enable and the record's tile must be the case's; the repeat must
also reproduce the first run bit for bit. Every output (out, out2, mask_out, out8, scale8) is
allocated with its padding and two spare rows and prefilled with a sentinel pattern, every
element is checked, and every pad column and spare row must come back untouched: a ragged tile
that writes past row M or column N fails here without faulting. Padding of the tensors the
epilogue reads (resid, the old out) holds NaN patterns, and mask_in random bits, so an index
built with the wrong leading dimension shows in the values.

Tolerances are gemm_ref's (the fp32 accumulation bound through the epilogue plus one fp16
rounding); ReLU bits are exact wherever the pre-activation is outside the bound, which leaves
at most 0.5 % of a case's elements open (tests/test_gemm_ref.py checks that from the reference)."""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as gr

pytestmark = pytest.mark.gpu

SENT16, SENT8 = 0x7D55, 0xA5   # an fp16 NaN pattern; a byte with mixed bits
CASES = gr.fused_cases()


def _upload_bytes(kf, arr):
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    host = np.full((a.size + 3) // 4 * 4, SENT8, np.uint8)
    host[:a.size] = a
    buf = kf.DeviceBuffer(host.size)
    kf.check(kf.core.bridge_transfer_int32(buf.ptr, host.ctypes.data, host.size // 4), "upload")
    return buf


def _read_bytes(kf, buf, n):
    return kf.read_fp16(buf.ptr, ((n + 3) // 4 * 2,)).view(np.uint8)[:n].copy()


def _padded16(live, rows, ld):
    """fp16 [rows x ld] of the sentinel with `live` in its top left corner"""
    host = np.full((rows, ld), SENT16, np.uint16)
    if live is not None:
        host[:live.shape[0], :live.shape[1]] = live.view(np.uint16)
    return host


def _operands(kf, c, ops):
    M, N, K, W = c["M"], c["N"], c["K"], ops["W"]
    keep = [kf.upload_fp16(ops["x"])]
    mk = {}
    if c["masked"]:
        keep.append(_upload_bytes(kf, ops["amask"]))
        mk = dict(mask=keep[-1].ptr, mask_rows=M)
    sp = ops["spec"]
    if sp["nparts"] == 1:
        a = kf.operand(keep[0].ptr, K, M, K, 1, **mk)
    else:
        a = kf.operand(keep[0].ptr, W, M, K, 1, nparts=2, part_width=W, tpolicy=sp["tpolicy"], dt=sp["dt"],
                       edges=list(sp["edges"]), **mk)
    B = ops["B"]
    if c["b"] == "rm":
        keep.append(kf.upload_fp16(B))
        b = kf.operand(keep[-1].ptr, N, K, N, 0)
    elif c["b"] == "kc":
        keep.append(kf.upload_fp16(B.T.copy()))
        b = kf.operand(keep[-1].ptr, K, N, K, 1)
    else:   # two-part k-contiguous view of a [2N x W] weight: B[n][p W + kk] = w[n + p N][kk]
        keep.append(kf.upload_fp16(np.concatenate([B[:W].T, B[W:].T], 0)))
        b = kf.operand(keep[-1].ptr, W, N, K, 1, nparts=2, part_width=W, T=2 * N, dt=(0, N))
    return a, b, keep


def _static(kf, c, d):
    """device copies of what the epilogue reads"""
    M = c["M"]
    s = {}
    if "bias" in d:
        s["bias"] = kf.upload_fp16(d["bias"])
    for k in ("scale", "shift", "scale2"):
        if k in d:
            s[k] = kf.upload_f32(d[k])
    if "resid" in d:
        s["resid"] = _upload_bytes(kf, _padded16(d["resid"], M, d["ldr"]))
    if "mask_in" in d:
        s["mask_in"] = _upload_bytes(kf, d["mask_in"])
    return s


def _launch(kf, c, d, a, b, s):
    """allocate and prefill the outputs, run the product, read everything back raw"""
    M, N, K = c["M"], c["N"], c["K"]
    R = M + 2
    sizes, bufs = {}, {}

    def out(name, host):
        sizes[name] = host.nbytes
        bufs[name] = _upload_bytes(kf, host)
        return bufs[name].ptr

    e = kf.KfEpilogue(alpha=d["alpha"], beta=d["beta"], relu=int(d["relu"]), resid_alpha=d["resid_alpha"])
    if d["has_out"]:
        e.out, e.ldo = out("out", _padded16(d.get("old"), R, d["ldo"])), d["ldo"]
    if c["epi"] == "fwd":
        e.mask_out, e.ldo = out("mask_out", np.full(R * d["ldo"] // 8, SENT8, np.uint8)), d["ldo"]
    if d["has_out2"]:
        e.out2, e.ldo2 = out("out2", _padded16(None, R, d["ldo2"])), d["ldo2"]
        e.scale2, e.mask_in = s["scale2"].ptr, s["mask_in"].ptr
    if d["has_out8"]:
        e.out8, e.ldo8 = out("out8", np.full(R * d["ldo8"], SENT8, np.uint8)), d["ldo8"]
        e.scale8, e.out8_src = out("scale8", np.full(R * d["ldo8"] // 32, SENT8, np.uint8)), d["out8_src"]
    if "bias" in s:
        e.bias = s["bias"].ptr
    if "scale" in s:
        e.scale, e.shift = s["scale"].ptr, s["shift"].ptr
    if "resid" in s:
        e.resid, e.ldr = s["resid"].ptr, d["ldr"]
    if c["edge"]:
        r0, r1, src = c["edge"]
        e.edge_out = out("edge", _padded16(None, 1, d["ldo"]))
        e.edge_r0, e.edge_r1, e.edge_src = r0, r1, src
    kf.check(kf.core.kf_gemm_fused(M, N, K, C.byref(a), C.byref(b), C.byref(e)), c["id"])
    if c["edge"]:   # what kf_rows_sum makes of the stored rows
        tgt, ld = (e.out2, e.ldo2) if c["edge"][2] else (e.out, e.ldo)
        ref = out("edge_ref", _padded16(None, 1, d["ldo"]))
        kf.check(kf.core.kf_rows_sum(ref, tgt, ld, c["edge"][0], c["edge"][1], N), "rows_sum")
    kf.sync()
    return {k: _read_bytes(kf, bufs[k], sizes[k]) for k in bufs}


def _within(got, ref, tol, what):
    bad = ~(np.abs(got - ref) <= tol)   # a NaN fails
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(),
                           float(np.nanmax(np.abs(got - ref) - tol)))


def _check16(raw, M, N, ld, ref, tol, what):
    got = raw.view(np.uint16).reshape(M + 2, ld)
    _within(np.ascontiguousarray(got[:M, :N]).view(np.float16).astype(np.float64), ref, tol, what)
    assert (got[:M, N:] == SENT16).all(), what + ": pad columns written"
    assert (got[M:] == SENT16).all(), what + ": rows past M written"


def _check(c, d, raw):
    M, N = c["M"], c["N"]
    ref = d["ref"]
    if d["has_out"]:
        _check16(raw["out"], M, N, d["ldo"], ref["v"], ref["tol"], "out")
    if d["has_out2"]:
        _check16(raw["out2"], M, N, d["ldo2"], ref["out2"], ref["tol2"], "out2")
    if d["relu"]:
        share = gr.relu_exempt_share(ref)
        print("%s: ReLU bits exempt %.5f %%" % (c["id"], 100 * share))
        assert share <= 0.005
    if "mask_out" in raw:
        ld = d["ldo"]
        bits = gr.unpack_bits(raw["mask_out"], M + 2, ld)
        sent = gr.unpack_bits(np.full(raw["mask_out"].size, SENT8, np.uint8), M + 2, ld)
        live, sure = bits[:M, :N], ref["sure"]
        assert np.array_equal(live[sure], ref["bits"][sure]), "ReLU mask bits"
        assert np.array_equal(bits[:M, N:], sent[:M, N:]), "mask_out: pad columns written"
        assert np.array_equal(bits[M:], sent[M:]), "mask_out: rows past M written"
    if d["has_out8"]:
        ld8 = d["ldo8"]
        codes = raw["out8"].reshape(M + 2, ld8)
        scales = raw["scale8"].reshape(M + 2, ld8 // 32)
        v, bound = (ref["out2"], ref["bound2"]) if d["out8_src"] else (ref["v"], ref["bound"])
        bad_s, bad_c = gr.mx_mismatch(np.ascontiguousarray(codes[:M, :N]), np.ascontiguousarray(scales[:M, :N // 32]),
                                      v, bound)
        assert not bad_s.any(), ("scale8", int(bad_s.sum()), np.argwhere(bad_s)[:4].tolist())
        assert not bad_c.any(), ("out8", int(bad_c.sum()), np.argwhere(bad_c)[:4].tolist())
        assert (codes[:M, N:] == SENT8).all() and (codes[M:] == SENT8).all(), "out8: padding written"
        assert (scales[:M, N // 32:] == SENT8).all() and (scales[M:] == SENT8).all(), "scale8: padding written"
    if c["edge"]:
        got, want = raw["edge"].view(np.uint16), raw["edge_ref"].view(np.uint16)
        assert np.array_equal(got[:N], want[:N]), "edge row differs from kf_rows_sum"
        assert not np.array_equal(got[:N], np.full(N, SENT16, np.uint16))
        assert (got[N:] == SENT16).all(), "edge_out: pad columns written"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_fused_tile(gpu, case):
    kf = gpu
    c = case
    d = gr.fused_inputs(c)
    a, b, keep = _operands(kf, c, d["ops"])
    s = _static(kf, c, d)
    raw = _launch(kf, c, d, a, b, s)
    _check(c, d, raw)
    # the identical call once more, profiled: the tile it ran on, and bit-identical results
    try:
        kf.core.kf_prof_reset()
        kf.core.kf_prof_enable(1)
        raw2 = _launch(kf, c, d, a, b, s)
        tiles = [r["tile"] for r in kf.prof_records() if r["cls"] == 0]
    finally:
        kf.core.kf_prof_reset()
        kf.core.kf_prof_enable(0)
    assert tiles == [c["tile"][0] * 10000 + c["tile"][1]], (tiles, c["tile"])
    for k in raw:
        assert np.array_equal(raw[k], raw2[k]), k + ": the repeated call differs"
    for buf in keep + list(s.values()):
        buf.free()
