"""float64 restatement of the conv operand rule of include/kf_ops.h (KfOperand with hout > 1:
the im2col of internal/nnet/forward.go:435-456 and its transposes), of the input-gradient
GEMMs host/backward.cpp builds on it, and the case tables of tests/test_gpu_conv_halo_elems.py.
No GPU needed: tests/test_conv_ref.py checks the rule and the cases' inputs from here alone.

Rule, per logical row r = (c, h), h < hout, and tap p = (dt, dh) (a part of `fin` columns):
  st = t0 + c * tmul + dt, zero outside [0, T);  sh = h * sub + dh, zero outside [0, hin)
  value = x[st][sh * fin + k]
The epilogue and the error bounds are tests/gemm_ref.py's (epilogue_ref, wgrad_tol).

Every case has two data sets. "int": x and dz in {-2..2}, W in {-1, 0, 1} at density 0.3, an
integer bias in [-3, 3] and scale2 in {0.5, 1, 2}: every pre-activation is an integer of at
most 2048 and every weight-gradient sum stays under 2^24, so fp16 / fp32 results are exact in
any summation order and the GPU comparison is array_equal. "gauss": unit-normal x / dz,
W ~ N(0, 1/K), bias in +-0.5 (the form of gemm_ref._operands), held to the per-element bound;
integer data cannot see a lost accumulator bit. At K = 2304 (256 channels) gemm_ref's
accumulation term K * 2^-23 * sum|a||b| would leave 0.63 % of the ReLU bits open, over the
project's 0.5 % cap, so the conv cases hold the kernels to half of it (ACC_TERMS): K * 2^-24 *
sum|a||b| still bounds any summation order of K exact products ((K - 1) u, u = 2^-24), every
element within it is within gemm_ref's bound, and the open share drops to 0.3 %.

Source buffers (`guarded`): two guard frames of 1000 before frame 0 and after frame T - 1, pad
columns of 1000 where the leading dimension is padded, all inside one allocation: a read that
should have been a zero shows as a gross error and can never fault. The operand's base
pointer is therefore always offset by whole frames.
"""
import functools

import numpy as np

from gemm_ref import epilogue_ref, h16, unpack_bits, wgrad_tol  # noqa: F401  (re-exported)

OFFS = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]
GUARD, GUARD_VAL = 2, 1000.0
PADW = 8           # pad columns of every output buffer
RELU_CAP = 0.005   # the project's cap on ReLU bits the bound leaves open
ACC_TERMS = 0.5    # the K passed to epilogue_ref, as a share of the product's K (above)


# ---------------------------------------------------------------- the operand rule
def im2col(x, T, hin, fin, hout, sub, offs, tmul=1, t0=0, nrows=None, ld=None):
    """[nrows x len(offs) * fin] float64 of the source frames x [T x ld] (ld = hin * fin unless
    given; columns past hin * fin are never read). nrows (default T * hout) logical rows: row
    (c, h) reads source frame t0 + c * tmul + dt."""
    ld = hin * fin if ld is None else ld
    xr = np.asarray(x, np.float64).reshape(T, ld)[:, :hin * fin].reshape(T, hin, fin)
    nrows = T * hout if nrows is None else nrows
    r = np.arange(nrows)
    c, h = r // hout, r % hout
    parts = []
    for dt, dh in offs:
        ts, hs = t0 + c * max(tmul, 1) + dt, h * sub + dh
        ok = (ts >= 0) & (ts < T) & (hs >= 0) & (hs < hin)
        parts.append(np.where(ok[:, None], xr[np.clip(ts, 0, T - 1), np.clip(hs, 0, hin - 1)], 0.0))
    return np.concatenate(parts, 1)


def col2im(dP, T, hin, fin, hout, sub, offs):
    """the transpose of im2col: dP [T * hout x len(offs) * fin] summed into [T * hin x fin]"""
    dx = np.zeros((T, hin, fin))
    r = np.arange(T * hout)
    t, h = r // hout, r % hout
    for o, (dt, dh) in enumerate(offs):
        ts, hs = t + dt, h * sub + dh
        ok = (ts >= 0) & (ts < T) & (hs >= 0) & (hs < hin)
        np.add.at(dx, (ts[ok], hs[ok]), np.asarray(dP, np.float64)[ok, o * fin:(o + 1) * fin])
    return dx.reshape(T * hin, fin)


# Input-gradient GEMMs (host/backward.cpp). Each is a list of taps (o, dt, dh): operand A
# gathers dz [frames x hout * fout] as an im2col with `rows_h` rows per frame, height stride 1
# and taps (dt, dh); operand B is op_wrows' B'[j][(p, n)] = W[o_p * fin + j][n].
def dgrad_plain_taps(offs):
    """conv_dgrad_plain: one transposed conv over all taps, rows_h = hin"""
    return [(o, -dt, -dh) for o, (dt, dh) in enumerate(offs)]


def dgrad_strided_taps(offs, sub, pi):
    """conv_dgrad_strided, residue pi: input height sub * j + pi receives only the taps with
    (pi - dh) % sub == 0; rows_h = hin / sub, output rows sub * m + pi"""
    return [(o, -dt, (pi - dh) // sub) for o, (dt, dh) in enumerate(offs) if (pi - dh) % sub == 0]


def dgrad_compact_taps(offs, e):
    """conv_dgrad_compact, residue e: input frame 3c + e receives only the taps with dt = e,
    from compact frame c; rows_h = hin, output rows grouped per frame (row_group / row_stride)"""
    return [(o, 0, -dh) for o, (dt, dh) in enumerate(offs) if dt == e]


def dgrad_gemm(dz, W, frames, rows_h, hsrc, fin, fout, taps):
    """(acc, mag) [frames * rows_h x fin] of one input-gradient GEMM over `taps`"""
    A = im2col(dz, frames, hsrc, fout, rows_h, 1, [(dt, dh) for _, dt, dh in taps])
    W = np.asarray(W, np.float64)
    Bt = np.concatenate([W[o * fin:(o + 1) * fin].T for o, _, _ in taps], 0)
    return A @ Bt, np.abs(A) @ np.abs(Bt)


def compact_ranges(T):
    """conv_dgrad_compact's residues without a tail: Tc0 compact frames 3c <= T - 1, and per
    e in (-1, 0, 1) the compact frames [c_lo, c_hi) whose input frame 3c + e exists"""
    tc0 = (T - 1) // 3 + 1
    return tc0, {e: (1 if e < 0 else 0, min(tc0, (T - 1 - e) // 3 + 1)) for e in (-1, 0, 1)}


# ---------------------------------------------------------------- buffers
def guarded(x, ld=None, guard_rows=None):
    """x [rows x w] -> (fp16 [guard + rows + guard x ld] with guards and pad columns of 1000,
    element offset of row 0). One frame per row of x unless guard_rows is given."""
    x = np.asarray(x)
    rows, w = x.shape
    ld = w if ld is None else ld
    g = GUARD if guard_rows is None else guard_rows
    buf = np.full((rows + 2 * g, ld), GUARD_VAL, np.float16)
    buf[g:g + rows, :w] = x
    return buf, g * ld


# ---------------------------------------------------------------- case tables
def _shape_id(s):
    return "%dx%dx%ds%dx%d" % (s[0], s[1], s[2], s[3], s[4])


def _geo_id(g):
    """fused geometry (BM, BN, nch, nbuf, pad, row tiles, column tiles)"""
    return "%dx%d-c%di%d-%s-%dx%d" % (g[0], g[1], g[2], g[3], "pad" if g[4] else "nopad", g[5], g[6])


def forward_cases():
    """dicts: id, shape (hin, fin, hout, sub, fout), T, tmul, t0, nc (output frames), ldpad,
    geo = (BM, BN, nch, nbuf, pitch pad, row tiles, column tiles)"""
    out = []

    def add(shape, T, geo, tmul=1, t0=0, nc=None, ldpad=0):
        nc = T if nc is None else nc
        cid = "fwd-%s-T%d" % (_shape_id(shape), T)
        if tmul > 1:
            cid += "-tmul%d-t%d-nc%d" % (tmul, t0, nc)
        if ldpad:
            cid += "-ld+%d" % ldpad
        out.append(dict(id=cid + "-" + _geo_id(geo), shape=shape, T=T, tmul=tmul, t0=t0, nc=nc, ldpad=ldpad, geo=geo))

    c2 = (40, 64, 40, 1, 64)
    add(c2, 52, (256, 64, 1, 1, 1, 9, 1))    # XCD remap, remainder 1, ragged last tile
    add(c2, 7, (256, 64, 1, 1, 1, 2, 1))     # no remap
    add(c2, 51, (256, 64, 1, 1, 1, 8, 1))    # remap, no remainder
    c16 = (16, 64, 16, 1, 64)                # M a whole number of tiles: tile edge on a frame edge
    add(c16, 16, (256, 64, 1, 1, 1, 1, 1))
    add(c16, 32, (256, 64, 1, 1, 1, 2, 1))
    add((20, 128, 20, 1, 128), 15, (256, 128, 2, 2, 1, 2, 1))   # two chunks, two images
    add((20, 128, 10, 2, 256), 29, (256, 256, 2, 1, 1, 2, 1))   # two chunks, one reloaded image
    add((10, 256, 10, 1, 256), 27, (256, 256, 4, 2, 0, 2, 1))   # four chunks, no pitch pad
    add((10, 64, 5, 2, 64), 53, (256, 64, 1, 1, 0, 2, 1))       # stride 2, odd hout: pad search gives up
    add((18, 128, 9, 2, 128), 31, (256, 128, 2, 1, 0, 2, 1))
    add((10, 64, 10, 1, 40), 27, (256, 64, 1, 1, 0, 2, 1))      # ragged column tile
    add((10, 64, 10, 1, 136), 27, (256, 256, 1, 1, 1, 2, 1))
    add((10, 64, 10, 1, 264), 27, (256, 256, 1, 1, 1, 2, 2))    # second column tile 8 wide
    for T in (1, 2):                                             # fewer frames than time taps
        add((10, 64, 10, 1, 64), T, (256, 64, 1, 1, 0, 1, 1))
        add((10, 256, 10, 1, 256), T, (256, 256, 4, 2, 0, 1, 1))
    add((10, 64, 10, 1, 64), 27, (256, 64, 1, 1, 0, 2, 1), ldpad=64)
    # time-strided rows: 128-row tiles. t0 = 0 with frame T - 1 unused; t0 = 2 ending on frame
    # T - 1, whose dt = +1 tap reads past the end
    for shape, nc, geo in (((10, 256, 10, 1, 256), 14, (128, 256, 4, 1, 1, 2, 1)),
                           ((10, 64, 10, 1, 64), 14, (128, 64, 1, 1, 0, 2, 1)),
                           ((20, 128, 20, 1, 128), 7, (128, 128, 2, 1, 1, 2, 1))):
        add(shape, 3 * (nc - 1) + 2, geo, tmul=3, t0=0, nc=nc)
        add(shape, 3 * (nc - 1) + 3, geo, tmul=3, t0=2, nc=nc)
    add((10, 64, 10, 1, 64), 28, (128, 64, 1, 1, 0, 2, 1), tmul=2, t0=1, nc=14)
    return out


def dgrad_cases():
    """dicts: id, kind ('plain' | 'strided' | 'compact'), shape, T, geo per call: (BM, BN, nch,
    nbuf, pad, row tiles, column tiles), in call order (residues 0, 1 / e = -1, 0, 1)"""
    out = []

    def add(kind, shape, T, geos):
        cid = "dgrad-%s-%s-T%d-%s" % (kind, _shape_id(shape), T, "+".join(_geo_id(g) for g in geos))
        out.append(dict(id=cid, kind=kind, shape=shape, T=T, geos=geos))

    # stride 1: nine taps on BROW 256-row tiles; the first with 9 tiles (XCD remap)
    add("plain", (40, 64, 40, 1, 64), 52, [(256, 64, 1, 1, 1, 9, 1)])
    add("plain", (20, 128, 20, 1, 128), 15, [(256, 128, 2, 2, 1, 2, 1)])
    add("plain", (10, 256, 10, 1, 256), 27, [(256, 256, 4, 2, 0, 2, 1)])
    # stride 2: residue 0 with 3 taps, residue 1 with 6, 128-row tiles; the first with 9 tiles
    add("strided", (40, 64, 20, 2, 128), 52, [(128, 64, 2, 2, 1, 9, 1), (128, 64, 2, 2, 0, 9, 1)])
    add("strided", (20, 128, 10, 2, 256), 27, [(128, 128, 4, 2, 1, 3, 1), (128, 128, 4, 2, 0, 3, 1)])
    add("strided", (10, 64, 5, 2, 64), 53, [(128, 64, 1, 1, 1, 3, 1), (128, 64, 1, 1, 1, 3, 1)])
    add("strided", (18, 128, 9, 2, 128), 31, [(128, 128, 2, 2, 1, 3, 1), (128, 128, 2, 2, 0, 3, 1)])
    # compact rows: three taps per residue e, rows grouped per frame
    add("compact", (10, 256, 10, 1, 256), 40, [(128, 256, 4, 2, 1, 2, 1)] * 3)
    add("compact", (20, 128, 20, 1, 128), 22, [(128, 128, 2, 2, 0, 2, 1)] * 3)
    return out


def wgrad_cases():
    """dicts: id, shape, T, bias, tail (t0, nt) or None, geo per call = (BN, waves, stages,
    splits, kps). T = 7: one split. The larger T: the smallest with two splits, nks % kps != 0
    and a reduction that is no multiple of 64; its K-steps straddle frames (64 % hout != 0) and
    K-step 5 starts on one (320 = 8 * 40 = 16 * 20 = 32 * 10)."""
    out = []

    def add(shape, T, geos, bias=True, tmul=1, tail=None):
        cid = "wgrad-%s-T%d" % (_shape_id(shape), T)
        if tmul > 1:
            cid += "-tmul%d-tail%d+%d" % (tmul, tail[0], tail[1])
        if not bias:
            cid += "-nobias"
        cid += "-" + "+".join("%dx-w%d-s%d-splits%d-kps%d" % g for g in geos)
        out.append(dict(id=cid, shape=shape, T=T, geos=geos, bias=bias, tmul=tmul, tail=tail))

    add((10, 256, 10, 1, 256), 7, [(64, 4, 3, 1, 2)])
    add((10, 256, 10, 1, 256), 103, [(64, 4, 3, 2, 9)])
    add((40, 64, 40, 1, 64), 7, [(64, 4, 2, 1, 5)])
    add((40, 64, 40, 1, 64), 26, [(64, 4, 2, 2, 9)])
    add((40, 64, 20, 2, 128), 7, [(128, 8, 2, 1, 3)])
    add((40, 64, 20, 2, 128), 52, [(128, 8, 2, 2, 9)])
    add((10, 256, 10, 1, 256), 7, [(64, 4, 3, 1, 2)], bias=False)
    # time-strided (conv_wgrad_compact): head frames 3c, then the tail frames 36, 39 (= T - 1)
    # with accumulate = 1 and B offset past the head rows
    add((10, 256, 10, 1, 256), 40, [(128, 8, 2, 1, 3), (128, 8, 2, 1, 1)], tmul=3, tail=(36, 2))
    return out


DATA = ("int", "gauss")


def _rng(c, data, salt=0):
    return np.random.default_rng([sum(map(ord, c["id"])), len(c["id"]), c["T"], int(data == "int"), salt])


def _draw(rng, data, shape, k=None):
    """source values; k: a weight matrix with that reduction length"""
    if data == "int":
        if k is None:
            return h16(rng.integers(-2, 3, shape))
        return h16(rng.integers(-1, 2, shape) * (rng.random(shape) < 0.3))
    v = rng.standard_normal(shape, dtype=np.float32)
    return h16(v if k is None else v / np.sqrt(k))


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=4)
def _forward_inputs(cid, data):
    c = next(x for x in forward_cases() if x["id"] == cid)
    hin, fin, hout, sub, fout = c["shape"]
    T, K, M = c["T"], 9 * fin, c["nc"] * hout
    rng = _rng(c, data)
    x = _draw(rng, data, (T, hin * fin))
    W = _draw(rng, data, (K, fout), K)
    bias = h16(rng.integers(-3, 4, fout)) if data == "int" else h16(rng.uniform(-0.5, 0.5, fout))
    A = im2col(x, T, hin, fin, hout, sub, OFFS, c["tmul"], c["t0"], M)
    W64 = W.astype(np.float64)
    ref = epilogue_ref(A @ W64, np.abs(A) @ np.abs(W64), ACC_TERMS * K, bias=bias, relu=True)
    return _freeze(dict(x=x, W=W, bias=bias, M=M, N=fout, K=K, ref=ref))


def forward_inputs(c, data):
    return _forward_inputs(c["id"], data)


def dgrad_calls(c):
    """the GEMM calls of a case: dicts of taps, frames (source frames of this call's A), f0
    (first source frame, compact only), rows_h, M, and out_rows (the dx row of each GEMM row)"""
    hin, fin, hout, sub, fout = c["shape"]
    T = c["T"]
    if c["kind"] == "plain":
        return [dict(taps=dgrad_plain_taps(OFFS), frames=T, f0=0, rows_h=hin, M=T * hin, out_rows=np.arange(T * hin))]
    if c["kind"] == "strided":
        return [dict(taps=dgrad_strided_taps(OFFS, sub, pi), frames=T, f0=0, rows_h=hin // sub, M=T * (hin // sub),
                     out_rows=sub * np.arange(T * (hin // sub)) + pi, pi=pi) for pi in range(sub)]
    tc0, rng_e = compact_ranges(T)
    calls = []
    for e in (-1, 0, 1):
        lo, hi = rng_e[e]
        m = np.arange((hi - lo) * hin)
        calls.append(dict(taps=dgrad_compact_taps(OFFS, e), frames=hi - lo, f0=lo, rows_h=hin, M=(hi - lo) * hin, e=e,
                          out_rows=(3 * (lo + m // hin) + e) * hin + m % hin))
    return calls


@functools.lru_cache(maxsize=4)
def _dgrad_inputs(cid, data):
    c = next(x for x in dgrad_cases() if x["id"] == cid)
    hin, fin, hout, sub, fout = c["shape"]
    T = c["T"]
    rng = _rng(c, data)
    frames = compact_ranges(T)[0] if c["kind"] == "compact" else T   # dz frames (compact: dzc)
    W = _draw(rng, data, (9 * fin, fout), 9 * fout)
    dz = _draw(rng, data, (frames, hout * fout))
    P = fin + PADW
    rows = T * hin
    scale2 = (2.0 ** rng.integers(-1, 2, fin)).astype(np.float32) if data == "int" else \
        rng.uniform(0.5, 1.5, fin).astype(np.float32)
    mask_in = rng.integers(0, 256, (rows + 2) * P // 8 + 4, dtype=np.uint8)   # random pad bits too
    mbits = unpack_bits(mask_in, rows, P)[:, :fin]
    calls = dgrad_calls(c)
    out2 = np.zeros((rows, fin))
    tol2 = np.zeros((rows, fin))
    owned = np.zeros(rows, bool)
    for call in calls:
        src = dz[call["f0"]:call["f0"] + call["frames"]]
        acc, mag = dgrad_gemm(src, W, call["frames"], call["rows_h"], hout, fin, fout, call["taps"])
        r = epilogue_ref(acc, mag, ACC_TERMS * len(call["taps"]) * fout, scale2=scale2, mask_in=mbits[call["out_rows"]])
        assert not owned[call["out_rows"]].any()
        owned[call["out_rows"]] = True
        out2[call["out_rows"]], tol2[call["out_rows"]] = r["out2"], r["tol2"]
        call["pre"] = acc
    # the whole gradient as one col2im, from the definition
    if c["kind"] == "compact":
        full = np.zeros((T, hout * fout))
        full[3 * np.arange(frames)] = dz.astype(np.float64)
    else:
        full = dz.astype(np.float64)
    dP = full.reshape(T * hout, fout) @ W.astype(np.float64).T
    whole = col2im(dP, T, hin, fin, hout, sub, OFFS) * scale2.astype(np.float64) * mbits
    return _freeze(dict(W=W, dz=dz, scale2=scale2, mask_in=mask_in, P=P, rows=rows, calls=calls, out2=out2, tol2=tol2,
                        owned=owned, whole=whole, frames=frames))


def dgrad_inputs(c, data):
    return _dgrad_inputs(c["id"], data)


def wgrad_calls(c):
    """(t0, tmul, frames) of each kf_gemm_wgrad call: the head (or the only call), then the tail"""
    if c["tmul"] == 1:
        return [(0, 1, c["T"])]
    return [(0, c["tmul"], (c["T"] - 1) // c["tmul"] + 1), (c["tail"][0], c["tmul"], c["tail"][1])]


@functools.lru_cache(maxsize=4)
def _wgrad_inputs(cid, data):
    c = next(x for x in wgrad_cases() if x["id"] == cid)
    hin, fin, hout, sub, fout = c["shape"]
    T = c["T"]
    rng = _rng(c, data)
    x = _draw(rng, data, (T, hin * fin))
    calls = wgrad_calls(c)
    rows = sum(n for _, _, n in calls) * hout
    dz = _draw(rng, data, (rows, fout))
    if data == "int":
        old_w = rng.integers(-8, 9, (9 * fin, fout)).astype(np.float32)
        old_b = rng.integers(-8, 9, fout).astype(np.float32)
    else:
        old_w = rng.standard_normal((9 * fin, fout), dtype=np.float32)
        old_b = rng.standard_normal(fout, dtype=np.float32)
    parts, r0 = [], 0
    for t0, tmul, n in calls:
        A = im2col(x, T, hin, fin, hout, sub, OFFS, tmul, t0, n * hout)
        B = dz[r0:r0 + n * hout].astype(np.float64)
        parts.append(dict(r0=r0, K=n * hout, acc=A.T @ B, mag=np.abs(A).T @ np.abs(B), bsum=B.sum(0),
                          bmag=np.abs(B).sum(0)))
        r0 += n * hout
    return _freeze(dict(x=x, dz=dz, old_w=old_w, old_b=old_b, parts=parts))


def wgrad_inputs(c, data):
    return _wgrad_inputs(c["id"], data)
