"""The restricted-attention kernels (k_att_fwd, k_att_bwd_q, k_att_bwd_kv through
kf_attention_forward / kf_attention_backward), element by element, over the geometries at
which their control flow changes (DESIGN §14 "Parity"; the matrix is attention_ref.CASES).

Every case runs at the dense pitch (ldp = H A, ldz = ldo = width) and at a padded, odd one
(ldp = H A + 3, ldz = width + 5, ldo = width + 1: rows not 4-byte aligned). Asserted:

  element bar   |got - r64| <= ulp16(r64) / 2 + 4 E32 per part (forward value / weight columns,
                the four parts of dproj): one fp16 rounding, plus 4 times the float32
                restatement's own worst error in the part, E32 = max(max |r32 - r64|,
                2^-24 max |r64|), for the kernels' other fp32 summation order (lane-split dot and
                butterfly, 8-wide blocks, key_scale after the sum) and expf against numpy's exp.
                The worst (|got - r64| - ulp16 / 2) / E32 is printed per part.
  exact zeros   where the float64 part is identically zero (context 1), got is zero exactly.
  ReLU mask     bits equal the reference's wherever |y64| > 4 E32 (at most 0.1 % left out,
                test_attention_ref.py); the byte of a partial last chunk like any other.
  nothing else  out, dproj, mask and scratch are prefilled with NaN sentinels and carry two guard
                rows / 16 guard bytes: every element of out[:T, :width] and dproj[:T, :H A] comes
                back finite, every pad column and guard bit-unchanged. A NaN scratch also shows
                that k_att_bwd_kv reads no word k_att_bwd_q did not write.
  determinism   a second backward gives a bit-identical dproj (gather, not scatter)."""
import ctypes as C

import numpy as np
import pytest

import attention_ref as AR
from attention_ref import CASES, CASE_IDS
from test_gpu_attention_kernel import KfAttention

pytestmark = pytest.mark.gpu

H16_SENT, F32_SENT = 0x7E5A, 0x7FC5A5A5   # a NaN in each format, as bits
FACTOR = 4.0


def _abi(kf):
    kf.core.kf_attention_forward.restype = C.c_int
    kf.core.kf_attention_forward.argtypes = [C.POINTER(KfAttention), C.c_void_p, C.c_longlong, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
    kf.core.kf_attention_backward.restype = C.c_int
    kf.core.kf_attention_backward.argtypes = [C.POINTER(KfAttention), C.c_void_p, C.c_longlong, C.c_void_p,
                                              C.c_void_p]


def _padded(a, ld, guard_rows=0):
    """fp16 [rows + guard_rows, ld] as bits: a in the leading columns, the sentinel elsewhere"""
    h = np.full((a.shape[0] + guard_rows, ld), H16_SENT, np.uint16)
    h[:a.shape[0], :a.shape[1]] = np.ascontiguousarray(a, np.float16).view(np.uint16)
    return h


class Run:
    """One geometry's device buffers at one pitch; forward() / backward() call the entry points
    and return the dense results after checking that nothing else was written."""

    def __init__(self, kf, case, inp, padded, use_mask=None):
        _abi(kf)
        self.kf, self.case = kf, case
        H, kd, vd, T, nl, nr, st = case
        self.ctx, self.A, self.od, self.width = AR.dims(H, kd, vd, nl, nr)
        self.HA = H * self.A
        self.ldp, self.ldz, self.ldo = ((self.HA + 3, self.width + 5, self.width + 1) if padded else
                                        (self.HA, self.width, self.width))
        self.dp = kf.upload_fp16(_padded(inp["proj"], self.ldp).view(np.float16))
        self.ddz = kf.upload_fp16(_padded(inp["dz"], self.ldz).view(np.float16))
        self.dscale, self.dshift = kf.upload_f32(inp["scale"]), kf.upload_f32(inp["shift"])
        self.use_mask = self.width % 8 == 0 if use_mask is None else use_mask
        self.att = KfAttention(self.dp.ptr, self.ldp, T, H, kd, vd, self.ctx, nl, st, inp["s"])

    def _fresh16(self, rows, ld):
        return self.kf.upload_fp16(np.full((rows, ld), H16_SENT, np.uint16).view(np.float16))

    def _dense16(self, buf, T, ld, used, what):
        """the [T, used] result of a [T + 2, ld] sentinel-prefilled buffer; pads and guards checked"""
        bits = self.kf.read_fp16(buf.ptr, (T + 2, ld)).view(np.uint16)
        assert (bits[T:] == H16_SENT).all(), f"{what}: a guard row was written"
        assert (bits[:T, used:] == H16_SENT).all(), f"{what}: a pad column was written"
        got = bits[:T, :used].view(np.float16)
        assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements not written or not finite"
        return got

    def forward(self):
        """(out fp16 [T, width], mask bits bool [T, width] or None)"""
        kf, T, width = self.kf, self.case[3], self.width
        out = self._fresh16(T + 2, self.ldo)
        mbuf, nb = None, T * width // 8
        if self.use_mask:
            mbuf = self._fresh16(1, (nb + 16 + 1) // 2)
        kf.check(kf.core.kf_attention_forward(C.byref(self.att), out.ptr, self.ldo, mbuf.ptr if mbuf else None,
                                              self.dscale.ptr, self.dshift.ptr), "attention fwd")
        got = self._dense16(out, T, self.ldo, width, "out")
        if not self.use_mask:
            return got, None
        n16 = (nb + 16 + 1) // 2
        raw = kf.read_fp16(mbuf.ptr, (n16,)).view(np.uint8)
        sent = np.full(n16, H16_SENT, np.uint16).view(np.uint8)
        assert np.array_equal(raw[nb:], sent[nb:]), "mask: a guard byte was written"
        return got, np.unpackbits(raw[:nb], bitorder="little").reshape(T, width).astype(bool)

    def backward(self):
        """(dproj fp16 [T, H A], scratch fp32 [2, T, H, ctx])"""
        kf, (H, kd, vd, T, nl, nr, st) = self.kf, self.case
        dproj = self._fresh16(T + 2, self.ldp)
        n = 2 * T * H * self.ctx
        scratch = kf.upload_f32(np.full(n + 4, F32_SENT, np.uint32).view(np.float32))
        kf.check(kf.core.kf_attention_backward(C.byref(self.att), self.ddz.ptr, self.ldz, dproj.ptr, scratch.ptr),
                 "attention bwd")
        got = self._dense16(dproj, T, self.ldp, self.HA, "dproj")
        sc = kf.read_f32(scratch.ptr, (n + 4,))
        assert (sc[n:].view(np.uint32) == F32_SENT).all(), "scratch: a guard word was written"
        assert np.isfinite(sc[:n]).all(), "scratch: a word k_att_bwd_q did not write"
        return got, sc[:n].reshape(2, T, H, self.ctx)


def check_elements(tag, case, ref, out, dproj):
    """The element bar and the exact zeros; returns {part: worst ratio} (printed by the caller)"""
    worst = {}
    for parts, got, k in ((AR.fwd_parts(case), out, "out"), (AR.bwd_parts(case), dproj, "g")):
        got = got.astype(np.float64)
        for name, sel in parts.items():
            r64, r32 = ref[k + "64"][:, sel], ref[k + "32"][:, sel]
            if k == "g" and r64.size and not r64.any():
                assert not got[:, sel].any(), (tag, name, "an exactly-zero part is not exactly zero")
            worst[name] = AR.element_excess(got[:, sel], r64, r32)
    print(tag, "worst (|got - r64| - ulp16/2) / E32:", {k: round(v, 3) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v > FACTOR}
    assert not bad, (tag, bad)
    return worst


def check_mask(tag, case, ref, bits, max_excluded=AR.MASK_EXCLUDED_MAX):
    inc = AR.mask_included(case, ref["y64"], ref["y32"])
    share = float((~inc).mean())
    print(tag, f"mask: {int((~inc).sum())} of {inc.size} bits left out ({100 * share:.3f} %)")
    assert share <= max_excluded, (tag, share)
    wrong = (bits != (ref["y64"] > 0)) & inc
    assert not wrong.any(), (tag, "wrong ReLU bits at (t, column)", np.argwhere(wrong)[:8].tolist())


REACHES = [
    "ctx 1: lg 6, all 64 lanes on one position; T 1; w == 1, three dproj parts exactly 0; width 17, mask NULL",
    "minimal key and value width (kd 1, vd 1), ctx 2: lg 5; width 3, mask NULL",
    "ctx 5: lg 3 with lanes 40-63 idle; T < span, every frame has dead positions; width 72 = one "
    "chunk + one mask byte",
    "T 3 < kWaves (idle waves); stride >= T, only the self position is live",
    "ctx 3: lg 4, lanes 48-63 idle; kd exactly one chunk; width 320 = 5 full chunks; T = 32 blocks + 2",
    "ctx 9: lg 2, a second 8-block with one real slot; kd two chunks; the key / value boundary inside "
    "a chunk of k_att_bwd_kv",
    "ctx 17: lg 1; right-only context (num_left 0); kd three chunks with a 2-column tail",
    "ctx 33: lg 0, 31 idle lanes; T far below ctx; four value chunks, the last partial",
    "ctx 64 and H ctx = 1024, the LDS limit; eight full 8-blocks",
    "value_dim 0; left-only (num_left = ctx - 1); width 15, mask NULL",
]


@pytest.mark.parametrize("pitch", ["dense", "padded"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_attention_geometry(gpu, i, pitch):
    """One geometry of the matrix at one pitch; REACHES[i] says which branch it reaches."""
    case = CASES[i]
    tag = f"{CASE_IDS[i]} {case} {pitch}"
    print(tag, "reaches:", REACHES[i])
    inp, ref = AR.case_reference(i)
    run = Run(gpu, case, inp, pitch == "padded")
    assert run.use_mask == (run.width % 8 == 0)
    out, bits = run.forward()
    dproj, _ = run.backward()
    check_elements(tag, case, ref, out, dproj)
    if bits is not None:
        check_mask(tag, case, ref, bits)
    again, _ = run.backward()
    assert np.array_equal(dproj.view(np.uint16), again.view(np.uint16)), "backward is not deterministic"


@pytest.mark.parametrize("which", ["every pair", "two pairs"])
def test_attention_sharp_softmax(gpu, which):
    """One position per sharpened (t, h) leads the next score by more than 120, beyond float32 exp
    underflow: the other weights are 0 in float32 and tiny but positive in float64. Outputs and
    gradients stay finite and meet the element bar.

    "every pair": geometry g3 with all 21 (t, h) sharp. Each sharp pair puts its ctx - 1 = 4
    underflowed weight columns under the mask rule's exclusion, 84 of 504 elements here, far above
    0.1 %, so at this size outputs and gradients are compared and the mask bits are not.
    "two pairs": g3's layer at T = 120 (8640 elements) with 2 sharp pairs, 8 excluded weight
    columns = 0.093 % of the case: the mask is compared under the rule, the share asserted."""
    H, kd, vd, T, nl, nr, st = CASES[2]
    if which == "every pair":
        case, pairs = CASES[2], None
    else:
        case, pairs = (H, kd, vd, 120, nl, nr, st), [(0, 1), (77, 2)]
    inp = AR.sharpen(case, AR.make_inputs(case, 31), pairs, 32, leader=None if pairs is None else nl)
    ref = AR.reference(case, inp)
    n_sharp = case[3] * H if pairs is None else len(pairs)
    w32 = ref["y32"][:, AR.fwd_parts(case)["forward weight"]]
    assert (w32 == 0).sum() >= 4 * n_sharp and (w32 == 1).sum() >= n_sharp   # the inputs are sharp
    run = Run(gpu, case, inp, False)
    out, bits = run.forward()
    dproj, _ = run.backward()
    check_elements(f"sharp, {which}", case, ref, out, dproj)
    if pairs is not None:
        check_mask(f"sharp, {which}", case, ref, bits)


# ---------------------------------------------------------------- refusals
_BASE = dict(H=2, kd=4, vd=4, T=4, ctx=3, nl=1, st=1)   # A 15, H A 30, width 14; with vd 5: width 16


def _refusals():
    """(id, entry points, field overrides, argument overrides): each must be refused on the host"""
    both = ("fwd", "bwd")
    return [
        ("context 65", both, dict(ctx=65, nl=40), {}),
        ("H ctx = 1025", both, dict(H=41, ctx=25, nl=12), {}),
        ("num_left = ctx", both, dict(nl=3), {}),
        ("num_left = -1", both, dict(nl=-1), {}),
        ("stride 0", both, dict(st=0), {}),
        ("T = 0", both, dict(T=0), {}),
        ("key_dim = 0", both, dict(kd=0), {}),
        ("ldp = H A - 1", both, {}, dict(ldp=-1)),
        ("ldo = width - 1", ("fwd",), {}, dict(ldo=-1)),
        ("ldz = width - 1", ("bwd",), {}, dict(ldz=-1)),
        ("mask with width % 8 != 0", ("fwd",), {}, dict(mask=True)),
        ("NULL proj", both, {}, dict(proj=None)),
        ("NULL out", ("fwd",), {}, dict(out=None)),
        ("NULL scale", ("fwd",), {}, dict(scale=None)),
        ("NULL dz", ("bwd",), {}, dict(dz=None)),
    ]


@pytest.mark.parametrize("name,entries,fields,args", _refusals(), ids=[r[0] for r in _refusals()])
def test_attention_refusals(gpu, name, entries, fields, args):
    """A host-side argument check (no kernel is launched): the call returns -1 with a message
    naming the entry point, leaves the sentinel-filled outputs bit-unchanged, and a valid call
    after it succeeds. The buffers are large enough for every refused shape all the same."""
    kf = gpu
    _abi(kf)
    NB = 1 << 16
    fill16 = np.full(NB // 2, H16_SENT, np.uint16).view(np.float16)
    proj = kf.upload_fp16(np.zeros(NB // 2, np.float16))
    dz = kf.upload_fp16(np.zeros(NB // 2, np.float16))
    scale, shift = kf.upload_f32(np.ones(NB // 4, np.float32)), kf.upload_f32(np.zeros(NB // 4, np.float32))
    out, dproj, mask = kf.upload_fp16(fill16), kf.upload_fp16(fill16), kf.upload_fp16(fill16)
    scratch = kf.upload_f32(np.full(NB // 4, F32_SENT, np.uint32).view(np.float32))

    def call(entry, g, a):
        A = 2 * g["kd"] + g["vd"] + g["ctx"]
        HA, width = g["H"] * A, g["H"] * (g["vd"] + g["ctx"])
        att = KfAttention(a.get("proj", proj.ptr), HA + a.get("ldp", 0), g["T"], g["H"], g["kd"], g["vd"], g["ctx"],
                          g["nl"], g["st"], 0.5)
        if entry == "fwd":
            return kf.core.kf_attention_forward(C.byref(att), a.get("out", out.ptr), width + a.get("ldo", 0),
                                                mask.ptr if a.get("mask") else None, a.get("scale", scale.ptr),
                                                shift.ptr)
        return kf.core.kf_attention_backward(C.byref(att), a.get("dz", dz.ptr), width + a.get("ldz", 0), dproj.ptr,
                                             scratch.ptr)

    for entry in entries:
        fn = b"kf_attention_forward" if entry == "fwd" else b"kf_attention_backward"
        assert call(entry, dict(_BASE, **fields), args) == -1, (name, entry, "was not refused")
        msg = kf.core.kf_last_error() or b""
        assert fn in msg, (name, entry, msg)
        for buf in (out, dproj, mask):
            assert (kf.read_fp16(buf.ptr, (NB // 2,)).view(np.uint16) == H16_SENT).all(), (name, entry, "wrote")
        assert (kf.read_f32(scratch.ptr, (NB // 4,)).view(np.uint32) == F32_SENT).all(), (name, entry, "wrote scratch")
        # a valid call after the refusal: width 16 with the mask (forward), or the backward
        kf.check(call(entry, dict(_BASE, vd=5), dict(mask=True)), "valid call after a refusal")
        kf.sync()
        buf = out if entry == "fwd" else dproj
        n = _BASE["T"] * (16 if entry == "fwd" else 2 * (2 * 4 + 5 + 3))
        assert np.isfinite(kf.read_fp16(buf.ptr, (n,))).all()
        for b in (out, dproj, mask):   # sentinels back for the next entry point
            kf.check(kf.core.bridge_transfer_fp16(b.ptr, fill16.ctypes.data, fill16.size), "refill")
        refill = np.full(NB // 4, F32_SENT, np.uint32)
        kf.check(kf.core.bridge_transfer_float32(scratch.ptr, refill.ctypes.data, refill.size), "refill")
