"""Float64 restatement of the semi-orthogonal constraint (kf_ops.h kf_orthonormal_constrain,
Kaldi's ConstrainOrthonormalInternal) for the tests, and the error bounds of the GPU kernel
derived from its accumulation lengths. Nothing here calls the kernel.

The rule, for W [K x n] (columns constrained) and a constraint value c:
    P = W^T W, nu = 0.125
    c < 0: tP = tr P, tPP = sum P_ij^2, s = sqrt(tPP / tP), ratio = tPP n / tP^2,
           nu *= 0.5 if ratio > 1.02, again if ratio > 1.1
    c > 0: s = c, ratio = 1
    Q = P - s^2 I, err = |Q|_F, W <- W - 4 (nu / s^2) W Q
A matrix with tP == 0 or a non-finite s stays untouched and reports s = 0.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24          # unit roundoff of fp32
KCHUNK = 512            # kf_ops.h KF_ORTHO_KCHUNK: rows of W per partial Gram tile


def ref_constrain(w, c):
    """w: float32 [K, n]; c: the constraint value. Returns a dict: w (float64 result), x (the
    update subtracted), P, Q, s, ratio, err, nu, factor, and margin, the relative distance of
    ratio from the nearer of the thresholds 1.02 and 1.1 (inf with a fixed scale)."""
    W = np.asarray(w, F32).astype(F64)
    n = W.shape[1]
    c = F64(F32(c))
    P = W.T @ W
    tP, tPP = np.trace(P), np.sum(P * P)
    nu, ratio, margin = 0.125, 1.0, np.inf
    untouched = dict(w=W, x=np.zeros_like(W), P=P, Q=None, s=0.0, ratio=0.0, err=0.0, nu=0.0, factor=0.0,
                     margin=np.inf)
    if c == 0 or tP == 0:
        return untouched
    if c < 0:
        s = np.sqrt(tPP / tP)
        ratio = tPP * n / tP ** 2
        margin = min(abs(ratio / 1.02 - 1), abs(ratio / 1.1 - 1))
        if ratio > 1.02:
            nu *= 0.5
        if ratio > 1.1:
            nu *= 0.5
    else:
        s = c
    if not np.isfinite(s):
        return untouched
    Q = P - s * s * np.eye(n)
    f = 4 * nu / (s * s)
    X = f * (W @ Q)
    return dict(w=W - X, x=X, P=P, Q=Q, s=s, ratio=ratio, err=np.sqrt(np.sum(Q * Q)), nu=nu, factor=f, margin=margin)


def rel_err(w, c=-1.0):
    """err / (s^2 sqrt(n)) of a matrix, in float64: 0 for a semi-orthogonal one"""
    r = ref_constrain(w, c)
    return r["err"] / (r["s"] ** 2 * np.sqrt(np.shape(w)[1]))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F32))).astype(F64)


def kernel_bounds(w, c, r):
    """Worst-case error bounds of the kernel against ref_constrain's result r, from its
    accumulation lengths (u = 2^-24, A = |W|^T |W|, every term a reference quantity):
      * P_ij is an fp32 fma chain over at most KCHUNK rows of W, the chunks' partials then added
        in fp32: dP_ij <= (min(K, KCHUNK) + chunks) u A_ij.
      * The traces are summed in double from that P: dtP <= sum dP_ii,
        dtPP <= sum (2 |P_ij| dP_ij + dP_ij^2). With a floating scale s^2 = tPP / tP, so
        d(s^2) / s^2 <= dtPP / tPP + dtP / tP =: e2, ds / s <= e2 / 2,
        dratio / ratio <= dtPP / tPP + 2 dtP / tP; with a fixed scale all three are 0. Each
        stat is then rounded to fp32: + u relative.
      * Q_ij = P_ij - s^2 [i == j] rounded to fp32: dQ_ij <= dP_ij + [i == j] s^2 e2 + u |Q_ij|,
        and |d err| <= |dQ|_F (triangle inequality) + u err.
      * X = f W Q with W Q an fp32 fma chain over n and f = 4 nu / s^2 rounded to fp32:
        dX <= f (|W| dQ + n u |W| |Q|) + (e2 + u) |X|, then w - f x costs one rounding of the
        product and one of the difference: u |X| + 1 ulp(w).
    Returns (ds, dratio, derr, dw [K x n])."""
    W = np.asarray(w, F32).astype(F64)
    K, n = W.shape
    aW = np.abs(W)
    A = aW.T @ aW
    chunks = -(-K // KCHUNK)
    dP = (min(K, KCHUNK) + chunks) * U * A
    P, Q = r["P"], r["Q"]
    if F32(c) < 0:
        dtP = np.trace(dP)
        dtPP = np.sum(2 * np.abs(P) * dP + dP * dP)
        tP, tPP = np.trace(P), np.sum(P * P)
        e2 = dtPP / tPP + dtP / tP
        dratio = r["ratio"] * (dtPP / tPP + 2 * dtP / tP + U)
    else:
        e2, dratio = 0.0, 0.0
    ds = r["s"] * (e2 / 2 + U)
    dQ = dP + np.eye(n) * (r["s"] ** 2 * e2) + U * np.abs(Q)
    derr = np.sqrt(np.sum(dQ * dQ)) + U * r["err"]
    X = np.abs(r["x"])
    dX = r["factor"] * (aW @ dQ + n * U * (aW @ np.abs(Q))) + (e2 + U) * X
    dw = dX + U * X + ulp32(r["w"])
    return ds, dratio, derr, dw


def gaussian(rng, K, n):
    return (rng.standard_normal((K, n)) / np.sqrt(K)).astype(F32)


def perm_columns(rng, K, n):
    """n columns of a K x K permutation matrix, float32"""
    w = np.zeros((K, n), F32)
    w[rng.permutation(K)[:n], np.arange(n)] = 1
    return w
