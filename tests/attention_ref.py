"""A plain numpy reference of the restricted attention (csrc/attention.hip's header), for any
geometry (H, kd, vd, T, num_left, num_right, stride, key_scale) and any dtype dt, and the
element bar the per-geometry kernel tests hold the kernels to.

Per frame t and head h the affine row holds [key (kd) | value (vd) | query key (kd) | query
context (ctx)]; position o attends row r_o = t + (o - num_left) * stride, zero outside [0, T):
    b_o = qctx[o] + key_scale <qkey(t), key(r_o)>,  w = softmax(b)
    y(t, h) = [sum_o w_o value(r_o) (vd) | w (ctx)],  out = relu(y) * scale + shift
tests/test_attention_ref.py pins att_forward to the oracle and att_backward to central finite
differences of att_forward, so neither rests on the kernels."""
import functools

import numpy as np

# (H, kd, vd, T, num_left, num_right, stride): the geometry matrix of DESIGN §14 "Parity"
CASES = [
    (1, 5, 16, 1, 0, 0, 1),
    (1, 1, 1, 2, 1, 0, 1),
    (3, 8, 19, 7, 2, 2, 3),
    (4, 16, 32, 3, 5, 2, 3),
    (5, 64, 61, 130, 1, 1, 1),
    (2, 72, 39, 37, 2, 6, 1),
    (2, 130, 3, 19, 0, 16, 2),
    (2, 24, 199, 5, 16, 16, 1),
    (16, 8, 8, 70, 40, 23, 1),
    (3, 16, 0, 9, 4, 0, 7),
]
CASE_IDS = [f"g{i + 1}" for i in range(len(CASES))]
MASK_EXCLUDED_MAX = 1e-3  # share of a case's elements the mask rule may leave out


def dims(H, kd, vd, nl, nr):
    """(ctx, A, od, width): context, per-head affine width, per-head output width, output width"""
    ctx = 1 + nl + nr
    return ctx, 2 * kd + vd + ctx, vd + ctx, H * (vd + ctx)


def _rows(T, ctx, nl, st):
    rows = np.arange(T)[:, None] + (np.arange(ctx)[None, :] - nl) * st          # [T, ctx]
    return (rows >= 0) & (rows < T), np.clip(rows, 0, T - 1)


def att_forward(proj, H, kd, vd, nl, nr, st, s, scale, shift, dt, rounded=False):
    """(y, out, bits): the pre-ReLU output [T, H (vd + ctx)] in dtype dt, relu(y) * scale + shift,
    and the ReLU decisions packed per row (bit k of byte b is column 8 b + k, as the kernel packs
    them). rounded: out after the single fp16 rounding the kernel makes (still in dt); False is
    the result before it."""
    T = proj.shape[0]
    ctx, A, od, width = dims(H, kd, vd, nl, nr)
    P = proj.astype(dt).reshape(T, H, A)
    y = np.zeros((T, H, od), dt)
    live, rc = _rows(T, ctx, nl, st)
    for h in range(H):
        key, val = P[:, h, :kd], P[:, h, kd:kd + vd]
        qk, qc = P[:, h, kd + vd:2 * kd + vd], P[:, h, 2 * kd + vd:]
        b = qc + dt(s) * np.where(live, np.einsum("td,tod->to", qk, key[rc]), dt(0))
        e = np.exp((b - b.max(1, keepdims=True)).astype(np.float64)).astype(dt)
        w = e / e.sum(1, keepdims=True, dtype=dt)
        y[:, h, :vd] = np.einsum("to,tod->td", np.where(live, w, dt(0)), val[rc])
        y[:, h, vd:] = w
    y = y.reshape(T, width)
    out = np.maximum(y, dt(0)) * np.asarray(scale, dt)[None, :] + np.asarray(shift, dt)[None, :]
    if rounded:
        out = out.astype(np.float16).astype(dt)
    return y, out, np.packbits(y > 0, axis=1, bitorder="little")


def att_backward(proj, dz, H, kd, vd, nl, nr, st, s, dt, rounded=False):
    """The exact gradient of the restricted attention (the kernel header's formulas) in
    dtype dt, in the oracle's loop order per (t, h). rounded: after the single fp16 rounding
    the kernels make (still in dt); False is the result before it."""
    T = proj.shape[0]
    ctx, A, od = 1 + nl + nr, 2 * kd + vd + 1 + nl + nr, vd + 1 + nl + nr
    P = proj.astype(dt).reshape(T, H, A)
    G = dz.astype(dt).reshape(T, H, od)
    dP = np.zeros_like(P)
    rows = np.arange(T)[:, None] + (np.arange(ctx)[None, :] - nl) * st          # [T, ctx]
    live = (rows >= 0) & (rows < T)
    rc = np.clip(rows, 0, T - 1)
    for h in range(H):
        key, val = P[:, h, :kd], P[:, h, kd:kd + vd]
        qk, qc = P[:, h, kd + vd:2 * kd + vd], P[:, h, 2 * kd + vd:]
        b = qc + dt(s) * np.where(live, np.einsum("td,tod->to", qk, key[rc]), dt(0))
        e = np.exp((b - b.max(1, keepdims=True)).astype(np.float64)).astype(dt)
        w = e / e.sum(1, keepdims=True, dtype=dt)
        gv, gw = G[:, h, :vd], G[:, h, vd:]
        dw = gw + np.where(live, np.einsum("td,tod->to", gv, val[rc]), dt(0))
        sw = (w * dw).sum(1, keepdims=True, dtype=dt)
        db = w * (dw - sw)
        dP[:, h, 2 * kd + vd:] = db
        dbl = np.where(live, db, dt(0))
        dP[:, h, kd + vd:2 * kd + vd] = dt(s) * np.einsum("to,tod->td", dbl, key[rc])
        for o in range(ctx):  # scatter to the attended rows
            ok = live[:, o]
            np.add.at(dP[:, h, :kd], rc[ok, o], dt(s) * dbl[ok, o, None] * qk[ok])
            np.add.at(dP[:, h, kd:kd + vd], rc[ok, o], w[ok, o, None] * gv[ok])
    dP = dP.reshape(T, H * A)
    return dP.astype(np.float16).astype(dt) if rounded else dP


# ---------------------------------------------------------------- inputs
def make_inputs(case, seed):
    """proj standard normal fp16, dz N(0, 0.05^2) at 60 % density (fp16), key_scale 1/sqrt(kd),
    scale / shift random fp32 per column with about a quarter of the scales negative."""
    H, kd, vd, T, nl, nr, st = case
    ctx, A, od, width = dims(H, kd, vd, nl, nr)
    rng = np.random.default_rng(seed)
    proj = rng.standard_normal((T, H * A)).astype(np.float16)
    dz = (rng.standard_normal((T, width)) * 0.05 * (rng.random((T, width)) < 0.6)).astype(np.float16)
    scale = (rng.uniform(0.5, 1.5, width) * np.where(rng.random(width) < 0.25, -1.0, 1.0)).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, width).astype(np.float32)
    return dict(proj=proj, dz=dz, s=float(np.float32(1.0 / np.sqrt(kd))), scale=scale, shift=shift)


def sharpen(case, inp, pairs, seed, leader=None):
    """Sharp softmax: in the given (t, h) pairs (None: all of them) one position's query context
    (leader; None: a random one, dead ones included) is 128 and the others' are -128 + N(0, 1)
    (fp16), so it leads the next score by far more than 120 (|key_scale <qkey, key>| stays in
    single digits): every other weight is 0 in float32 (exp underflows) and tiny but positive in
    float64."""
    H, kd, vd, T, nl, nr, st = case
    ctx, A, od, width = dims(H, kd, vd, nl, nr)
    rng = np.random.default_rng(seed)
    P = inp["proj"].copy().reshape(T, H, A)
    if pairs is None:
        pairs = [(t, h) for t in range(T) for h in range(H)]
    for t, h in pairs:
        qc = (-128.0 + rng.standard_normal(ctx)).astype(np.float16)
        qc[rng.integers(ctx) if leader is None else leader] = 128.0
        P[t, h, 2 * kd + vd:] = qc
    return dict(inp, proj=P.reshape(T, H * A))


def reference(case, inp):
    """The float64 reference and its unrounded float32 restatement on given inputs:
    y / out / bits (forward) and g (dproj), suffixed 64 and 32."""
    H, kd, vd, T, nl, nr, st = case
    r = {}
    for dt, k in ((np.float64, "64"), (np.float32, "32")):
        y, out, bits = att_forward(inp["proj"], H, kd, vd, nl, nr, st, inp["s"], inp["scale"], inp["shift"], dt)
        r["y" + k], r["out" + k], r["bits" + k] = y.astype(np.float64), out.astype(np.float64), bits
        r["g" + k] = att_backward(inp["proj"], inp["dz"], H, kd, vd, nl, nr, st, inp["s"], dt).astype(np.float64)
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def case_reference(i):
    """(inputs, reference) of CASES[i] on its seeded inputs, computed once and shared"""
    inp = make_inputs(CASES[i], 100 + i)
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return inp, reference(CASES[i], inp)


# ---------------------------------------------------------------- the element bar
def fwd_parts(case):
    """name -> boolean column selection of the output row [H (vd + ctx)]"""
    H, kd, vd, T, nl, nr, st = case
    ctx, A, od, width = dims(H, kd, vd, nl, nr)
    j = np.arange(width) % od
    return {"forward value": j < vd, "forward weight": j >= vd}


def bwd_parts(case):
    """name -> boolean column selection of the dproj row [H A]"""
    H, kd, vd, T, nl, nr, st = case
    ctx, A, od, width = dims(H, kd, vd, nl, nr)
    j = np.arange(H * A) % A
    return {"key": j < kd, "value": (j >= kd) & (j < kd + vd), "query key": (j >= kd + vd) & (j < 2 * kd + vd),
            "query context": j >= 2 * kd + vd}


def ulp16(x):
    """the fp16 spacing at |x|: 2^(floor(log2 |x|) - 10), and 2^-24 below 2^-14"""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def e32_of(r32, r64):
    """E32 of a part: max(max |r32 - r64|, 2^-24 max |r64|); 0 for an empty or all-zero part"""
    if r64.size == 0:
        return 0.0
    return float(max(np.abs(r32 - r64).max(), 2.0 ** -24 * np.abs(r64).max()))


def element_excess(got, r64, r32):
    """The worst (|got - r64| - ulp16(r64) / 2) / E32 over a part (the bar is <= 4); 0 where no
    element exceeds the rounding term, inf where one does and E32 is 0 (an exact-zero part)."""
    if r64.size == 0:
        return 0.0
    over = (np.abs(np.asarray(got, np.float64) - r64) - 0.5 * ulp16(r64)).max()
    if over <= 0:
        return 0.0
    e32 = e32_of(r32, r64)
    return float(over / e32) if e32 > 0 else float("inf")


def mask_included(case, y64, y32):
    """[T, width] bool: the elements whose ReLU bit is compared, |y64| > 4 E32, E32 per forward
    part of the pre-ReLU output"""
    inc = np.zeros(y64.shape, bool)
    for sel in fwd_parts(case).values():
        inc[:, sel] = np.abs(y64[:, sel]) > 4 * e32_of(y32[:, sel], y64[:, sel])
    return inc
