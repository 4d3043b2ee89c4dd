"""Float64 numpy restatement of the online natural-gradient preconditioner (Povey,
Zhang, Khudanpur, "Parallel training of DNNs with natural gradient and parameter averaging", the
online variant) for the tests. It shares no code with csrc/natgrad.hip and is checked on its own
in tests/test_natgrad_ref.py before anything is compared with it.

One preconditioner works on row vectors of dimension D with rank R; its state is W [R x D], d [R],
rho and the step count t. For a minibatch X [N x D]:

    eta  = min(0.9, 1 - exp(-N / num_samples_history))
    beta = rho (1 + alpha) + alpha sum(d) / D;  e_i = 1 / (beta / d_i + 1)     (W = E^1/2 R_t)
    H = X W^T;  L = H^T H;  trX = tr(X X^T)
    Xh = X - H W;  tr(Xh Xh^T) = trX - sum_i (2 - e_i) L_ii
    gamma = sqrt(trX / tr(Xh Xh^T))   (1 if either trace is 0 or not finite);  output gamma Xh

and on an updating step (t < 10 or t % update_period == 0), after the output is formed:

    J = H^T X;  K = J J^T;  Dr = diag(d) + rho I;  F = E^-1/2
    Z = (eta/N)^2 F K F + (eta/N)(1 - eta)(Dr F L F + F L F Dr) + (1 - eta)^2 Dr^2
    Z = U diag(c) U^T, c descending;  c_i = max(c_i, (rho (1 - eta))^2);  s = sqrt(c)
    rho' = max(eps, ((eta/N) trX + (1 - eta)(D rho + sum(d)) - sum(s)) / (D - R))
    d'_i = max(s_i - rho', eps, delta max_j (s_j - rho'))
    R' = diag(1/s) U^T ((eta/N) F J + (1 - eta) Dr F W);  W' = E'^1/2 R'
"""
import numpy as np

F64 = np.float64
DEFAULTS = dict(update_period=4, num_samples_history=2000.0, alpha=4.0, epsilon=1e-10, delta=5e-4)


def e_of(d, rho, D, alpha):
    beta = rho * (1.0 + alpha) + alpha * d.sum() / D
    return 1.0 / (beta / d + 1.0)


class Pre:
    def __init__(self, D, R, **opts):
        self.D, self.R = D, R
        self.o = dict(DEFAULTS, **opts)
        eps = F64(np.float32(self.o["epsilon"]))          # the options travel as fp32
        self.o["epsilon"], self.o["delta"] = eps, F64(np.float32(self.o["delta"]))
        self.rho, self.d, self.t = eps, np.full(R, eps, F64), 0
        r0 = np.zeros((R, D), F64)
        for j in range(D):
            r0[j % R, j] = 1.0 / np.sqrt(np.ceil(D / R))
        r0 /= np.linalg.norm(r0, axis=1, keepdims=True)
        self.W = np.sqrt(self.e())[:, None] * r0

    def copy(self):
        c = Pre.__new__(Pre)
        c.D, c.R, c.o, c.rho, c.t = self.D, self.R, dict(self.o), self.rho, self.t
        c.d, c.W = self.d.copy(), self.W.copy()
        return c

    def e(self):
        return e_of(self.d, self.rho, self.D, self.o["alpha"])

    def rt(self):
        """R_t recovered from W"""
        return self.W / np.sqrt(self.e())[:, None]

    def proj(self):
        return self.W.T @ self.W

    def updating(self):
        return self.t < 10 or self.t % self.o["update_period"] == 0

    def eta(self, N):
        return min(0.9, 1.0 - np.exp(-N / self.o["num_samples_history"]))

    def gamma(self, trx, ldiag):
        trh = trx - np.sum((2.0 - self.e()) * ldiag)
        if not (np.isfinite(trx) and np.isfinite(trh) and trx > 0 and trh > 0):
            return 1.0
        return float(np.sqrt(trx / trh))

    def stats(self, X):
        X = np.asarray(X, F64)
        H = X @ self.W.T
        J = H.T @ X
        return dict(H=H, L=H.T @ H, J=J, K=J @ J.T, trx=float(np.sum(X * X)), N=X.shape[0])

    def build_z(self, L, K, N):
        eta = self.eta(N)
        a, b = eta / N, 1.0 - eta
        f = 1.0 / np.sqrt(self.e())
        dr = self.d + self.rho
        flf = f[:, None] * L * f[None, :]
        Z = a * a * (f[:, None] * K * f[None, :]) + a * b * (dr[:, None] * flf + flf * dr[None, :]) + b * b * np.diag(dr * dr)
        return 0.5 * (Z + Z.T), a, b, f, dr

    def update_from_stats(self, L, K, J, trx, N):
        """the state update from given statistics; returns what was decided on the way"""
        D, R, o = self.D, self.R, self.o
        Z, a, b, f, dr = self.build_z(np.asarray(L, F64), np.asarray(K, F64), N)
        c, U = np.linalg.eigh(Z)
        c, U = c[::-1], U[:, ::-1]
        raw = c.copy()
        floor = (self.rho * b) ** 2
        c = np.maximum(c, floor)
        s = np.sqrt(c)
        rho1 = max(o["epsilon"], (a * trx + b * (D * self.rho + self.d.sum()) - s.sum()) / (D - R))
        d1 = np.maximum(np.maximum(s - rho1, o["epsilon"]), o["delta"] * np.max(s - rho1))
        M = a * f[:, None] * np.asarray(J, F64) + b * (dr * f)[:, None] * self.W
        R1 = (U.T @ M) / s[:, None]
        self.rho, self.d = float(rho1), d1
        self.W = np.sqrt(self.e())[:, None] * R1
        return dict(raw=raw, floor=floor, floored=int(np.sum(raw < floor)), s=s)

    def step(self, X):
        """precondition X, then update the state if this is an updating step; returns gamma Xh, gamma"""
        X = np.asarray(X, F64)
        st = self.stats(X)
        g = self.gamma(st["trx"], np.diag(st["L"]))
        out = g * (X - st["H"] @ self.W)
        if self.updating():
            self.update_from_stats(st["L"], st["K"], st["J"], st["trx"], st["N"])
        self.t += 1
        return out, g


def low_rank_batch(rng, N, D, basis, noise=0.05):
    """N rows in the span of basis' rows (scales falling from 3 to 1) plus isotropic noise"""
    k = basis.shape[0]
    return (rng.standard_normal((N, k)) * np.linspace(3.0, 1.0, k)) @ basis + noise * rng.standard_normal((N, D))


def precondition_gradient(G, gin, gout, Pin, Pout):
    """gamma_in gamma_out (I - W_in^T W_in) G (I - W_out^T W_out); a side given as None is left alone"""
    G = np.asarray(G, F64)
    if Pin is not None:
        G = G - Pin @ G
    if Pout is not None:
        G = G - G @ Pout
    return gin * gout * G


def operand_rows(x, nrows, T, dts, policy_clamp, edges=()):
    """the logical matrix of a spliced operand (kf_ops.h KfOperand, hout = 1) materialised in
    float64: part p of row t is source row t + dt[p], clamped into or zero outside [0, T), or the
    edge row where (p, t, row) is listed"""
    x = np.asarray(x, F64)
    w = x.shape[1]
    out = np.zeros((nrows, len(dts) * w), F64)
    edge = {(p, t): row for p, t, row in edges}
    for t in range(nrows):
        for p, dt in enumerate(dts):
            if (p, t) in edge:
                st = edge[(p, t)]
            else:
                st = t + dt
                if st < 0 or st >= T:
                    if not policy_clamp:
                        continue
                    st = min(max(st, 0), T - 1)
            out[t, p * w:(p + 1) * w] = x[st]
    return out
