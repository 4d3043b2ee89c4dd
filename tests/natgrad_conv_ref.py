"""Float64 restatement of the parameter-side natural gradient of the conv components (DESIGN §32;
Kaldi's TimeHeightConvolutionComponent) on top of natgrad_ref.Pre. It shares no code with
csrc/natgrad_conv.hip and is checked on its own in tests/test_natgrad_conv_ref.py.

G = [dW ; db] is [Din x N]. The in side's data are the N rows of G^T, the out side's the Din rows
of G1 = G - W_in^T W_in G, which is passed on without gamma_in; both scalars go in at the end:
G^ = gamma_in gamma_out (G1 - G1 W_out^T W_out). The history is counted in minibatches:
num_samples_history = num_minibatches_history x (rows of X), so eta = 1 - exp(-1 / that) on both sides.
"""
import numpy as np

from natgrad_ref import F64, Pre


def clamped_rank(want, dim, max_rank=96):
    r = min(want, dim // 2, max_rank)
    return r if r >= 8 else 0


class ConvPre:
    def __init__(self, Din, N, rank_in=80, rank_out=80, num_minibatches_history=4.0, **opts):
        rin, rout = clamped_rank(rank_in, Din), clamped_rank(rank_out, N)
        self.pin = Pre(Din, rin, num_samples_history=num_minibatches_history * N, **opts) if rin else None
        self.pout = Pre(N, rout, num_samples_history=num_minibatches_history * Din, **opts) if rout else None

    def sides(self):
        return [p for p in (self.pin, self.pout) if p is not None]

    def step(self, G):
        """returns G^, and per side ("in" / "out") its gamma and statistics; then the state update"""
        G = np.asarray(G, F64)
        info, cur, scale = {}, G.T, 1.0
        for name, p in (("in", self.pin), ("out", self.pout)):
            if p is not None:
                st = p.stats(cur)
                g = p.gamma(st["trx"], np.diag(st["L"]))
                info[name] = dict(st, gamma=g)
                cur, scale = cur - st["H"] @ p.W, scale * g
            cur = cur.T      # the in side works on G^T, the out side on G1
        for name, p in (("in", self.pin), ("out", self.pout)):
            if p is not None:
                st = info[name]
                if p.updating():
                    p.update_from_stats(st["L"], st["K"], st["J"], st["trx"], st["N"])
                p.t += 1
        return scale * cur.T, info
