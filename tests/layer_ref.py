"""Plain numpy references of the non-MFMA layer and ivector operations declared in
include/kf_ops.h (csrc/layers.hip, csrc/ivector.hip), written from the contract text there
and not from the kernels. fp64 unless stated; inputs are taken as given (callers pass the
fp16-rounded values they upload). tests/test_layer_ref.py checks these against each other on
the CPU; the GPU tests compare the kernels with them."""
import numpy as np

F16_ULP = 2.0 ** -10   # relative spacing of fp16 normals
F32_U = 2.0 ** -24     # fp32 unit roundoff, also the fp16 subnormal spacing


def f64(a):
    return np.asarray(a, np.float64)


def acc_bound(n_terms, abs_sum, ref=None):
    """|got - ref| allowed for an fp32 accumulation of n_terms terms whose absolute values
    sum to abs_sum, stored as fp16 (ref given: plus one fp16 ulp of it) or as fp32."""
    b = np.maximum(n_terms, 1) * F32_U * f64(abs_sum) + F32_U
    if ref is not None:
        b = b + F16_ULP * np.abs(f64(ref))
    return b


def taps(dts, dhs):
    """the dt x dh cross product of a conv's offsets, dt-major"""
    return [d for d in dts for _ in dhs], [h for _ in dts for h in dhs]


T3 = (-1, 0, 1)
# (T, hin, hout, sub, fout, dts, dhs) of the one-input-filter conv tests
C1_GEOMS = [
    (1, 40, 40, 1, 32, T3, T3),
    (16, 40, 40, 1, 64, T3, T3),
    (17, 40, 40, 1, 8, T3, T3),
    (37, 40, 20, 2, 64, T3, T3),
    (33, 10, 8, 1, 256, (0,), (0, 1, 2)),
    (21, 12, 12, 1, 16, (0, 1), (0,)),
    (19, 9, 9, 1, 128, (-2, 0, 2), (-1, 1)),
]


# ---------------------------------------------------------------- bit masks
def pack_bits(bits):
    """bit i of byte i/8 = bits.flat[i]"""
    return np.packbits(np.asarray(bits, bool).reshape(-1), bitorder="little")


def unpack_bits(packed, n):
    return np.unpackbits(np.asarray(packed, np.uint8), bitorder="little")[:n].astype(bool)


# ---------------------------------------------------------------- row sets
def compact_rows(T, tc0, tc):
    """source row of compact row c: 3c for c < tc0, else (T-1) - 3(tc-1-c)"""
    return np.array([3 * c if c < tc0 else (T - 1) - 3 * (tc - 1 - c) for c in range(tc)], np.int64)


def gather_rows(src, T, tc0, tc):
    return np.asarray(src)[compact_rows(T, tc0, tc)]


def scatter_rows(src, T, tc0, tc, r0=0):
    """full rows r0 .. T-1: the compact row of src whose source row it is, or zeros"""
    src = np.asarray(src)
    dst = np.zeros((T - r0,) + src.shape[1:], src.dtype)
    for c, row in enumerate(compact_rows(T, tc0, tc)):
        if row >= r0:
            dst[row - r0] = src[c]
    return dst


def rows_sum(src, rows, mask=None):
    """fp32 sum of src[r] over rows in the given order (masked-out elements skipped), then
    one rounding to fp16"""
    src = np.asarray(src, np.float16)
    s = np.zeros(src.shape[1], np.float32)
    for r in rows:
        nxt = s + src[r].astype(np.float32)
        s = nxt if mask is None else np.where(np.asarray(mask, bool)[r], nxt, s)
    return s.astype(np.float16)


# ---------------------------------------------------------------- conv with one input filter
def conv_c1(x, W, bias, scale, shift, T, hin, hout, sub, dt, dh):
    """x [T x hin], W [noff x fout]; row (t, h) of the result is frame t, height h.
    pre = bias + sum_o x[t + dt[o]][h*sub + dh[o]] W[o] (zero outside the input),
    mask = pre > 0, y = max(pre, 0) * scale + shift. Returns (pre, mask, y), [T*hout x fout]."""
    x, W = f64(x).reshape(T, hin), f64(W)
    fout = W.shape[1]
    pre = np.zeros((T, hout, fout))
    if bias is not None:
        pre += f64(bias)
    for o in range(len(dt)):
        hs = np.arange(hout) * sub + dh[o]
        ok = (hs >= 0) & (hs < hin)
        for t in range(T):
            ts = t + dt[o]
            if 0 <= ts < T:
                pre[t, ok] += x[ts, hs[ok]][:, None] * W[o][None, :]
    pre = pre.reshape(T * hout, fout)
    mask = pre > 0
    y = np.where(mask, pre, 0.0)
    if scale is not None:
        y = y * f64(scale) + f64(shift)
    return pre, mask, y


def conv_c1_wgrad(x, dz, T, hin, hout, sub, dt, dh):
    """dW[o][f] = sum over rows (t, h) of x[t + dt[o]][h*sub + dh[o]] dz[(t, h)][f],
    db[f] = sum over rows of dz"""
    x = f64(x).reshape(T, hin)
    dz = f64(dz).reshape(T, hout, -1)
    dW = np.zeros((len(dt), dz.shape[2]))
    for o in range(len(dt)):
        for t in range(T):
            for h in range(hout):
                ts, hs = t + dt[o], h * sub + dh[o]
                if 0 <= ts < T and 0 <= hs < hin:
                    dW[o] += x[ts, hs] * dz[t, h]
    return dW, dz.sum(axis=(0, 1))


# ---------------------------------------------------------------- ivector input path
def combine_fm(a, b, seq_off, T, height, nf1, nf2):
    """out[t][h*(nf1+nf2) + f] = f < nf1 ? a[t][h*nf1 + f] : b[seq(t)][h*nf2 + f - nf1];
    seq_off None: b has one row per frame"""
    a = np.asarray(a).reshape(T, height, nf1)
    b = np.asarray(b)
    out = np.zeros((T, height, nf1 + nf2), a.dtype)
    out[:, :, :nf1] = a
    if seq_off is None:
        out[:, :, nf1:] = b.reshape(T, height, nf2)
    else:
        for s in range(len(seq_off) - 1):
            out[seq_off[s]:seq_off[s + 1], :, nf1:] = b[s].reshape(height, nf2)
    return out.reshape(T, height * (nf1 + nf2))


def combine_fm_bwd(dy, seq_off, height, nf1, nf2):
    """db[s][h*nf2 + g] = sum over the frames t of sequence s of dy[t][h*(nf1+nf2) + nf1 + g]"""
    dy = f64(dy).reshape(-1, height, nf1 + nf2)
    B = len(seq_off) - 1
    db = np.zeros((B, height * nf2))
    for s in range(B):
        for t in range(seq_off[s], seq_off[s + 1]):
            db[s] += dy[t, :, nf1:].reshape(-1)
    return db


def im2col_small(x, T, hin, hout, sub, fin, dt, dh, kp):
    """P [T*hout x kp]: column tap*fin + c = x[t + dt[tap]][ho*sub + dh[tap]][c], zero outside
    the input and in columns >= ntaps*fin"""
    x = np.asarray(x).reshape(T, hin, fin)
    P = np.zeros((T * hout, kp), x.dtype)
    for t in range(T):
        for ho in range(hout):
            for tap in range(len(dt)):
                ts, hs = t + dt[tap], ho * sub + dh[tap]
                if 0 <= ts < T and 0 <= hs < hin:
                    P[t * hout + ho, tap * fin:(tap + 1) * fin] = x[ts, hs]
    return P


def col2im_small(dP, T, hin, hout, sub, fin, dt, dh, kp):
    """the transpose of im2col_small: dx [T x hin*fin] (fp64)"""
    dP = f64(dP).reshape(T * hout, kp)
    dx = np.zeros((T, hin, fin))
    for t in range(T):
        for ho in range(hout):
            for tap in range(len(dt)):
                ts, hs = t + dt[tap], ho * sub + dh[tap]
                if 0 <= ts < T and 0 <= hs < hin:
                    dx[ts, hs] += dP[t * hout + ho, tap * fin:(tap + 1) * fin]
    return dx.reshape(T, hin * fin)


# ---------------------------------------------------------------- flat SGD
def sgd_flat(w, g, v, lr, mom):
    """v' = mom*v + g; w' = w - lr*v'. Returns (w', v')."""
    v1 = float(mom) * f64(v) + f64(g)
    return f64(w) - float(lr) * v1, v1
