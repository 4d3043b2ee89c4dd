"""float64 reference of the chain xent derivative and objective (kf_chain.h kf_chain_xent,
DESIGN §26), from the numerator posteriors of tests/chain_ref.py. No GPU needed:
tests/test_xent_ref.py pins it to torch's float64 autograd.

For every supervised frame, with post the numerator posteriors [T x P] (chain_ref.num_f64
already drops labels <= 0 and > P) and y the log-softmax output:
    S    = sum_p post[p]                                  (the computed sum, not 1)
    grad = -xr * w * (post - exp(y) * S)                  the loss gradient at the affine output
    objf = w * sum_t sum_p post * y
a sequence whose chain objective is not finite (ok = 0) gives zeros for both.
`shift` and `with_s` are the mutations of test_xent_ref.py: the pdf map off by one, and the S
term exp(y) * S dropped. (S itself is 1 to rounding whenever the total is finite: the posteriors
of a frame sum to one over the arcs that are kept. Only the term's presence can be tested, not
whether the computed sum or 1 multiplies it.)
"""
import numpy as np

import chain_ref as cr


def log_softmax_f64(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def xent_outputs(seed, T, P, scale=2.0):
    """fp16 log-softmax rows [T x P] of random logits (standard_normal * scale)."""
    z = np.random.default_rng(seed).standard_normal((T, P)) * scale
    return log_softmax_f64(z).astype(np.float16)


def xent_from_post(post, y, xr, w, ok=True, shift=0, with_s=True):
    """(grad [T x P], objf) from dense posteriors."""
    post = np.asarray(post, np.float64)
    y = np.asarray(y, np.float64)
    if not ok:
        return np.zeros_like(post), 0.0
    if shift:
        post = np.roll(post, shift, axis=1)
    S = post.sum(axis=1, keepdims=True) if with_s else 0.0
    grad = -xr * w * (post - np.exp(y) * S)
    pos = post != 0                       # (0 * -inf: a pdf without posterior adds nothing)
    objf = w * float(np.sum(post[pos] * y[pos]))
    return grad, objf


def xent_f64(f, x, y, xr, w, ok=None, **mut):
    """(grad, objf, weight) of one sequence: FST f on chain outputs x [T x P], xent outputs y.
    ok None: the numerator's total is finite (the den side is the caller's to judge)."""
    x = np.asarray(x, np.float64)
    T = x.shape[0]
    if T == 0:
        return np.zeros_like(x), 0.0, 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        total, post = cr.num_f64(f, x)
    if ok is None:
        ok = bool(np.isfinite(total))
    grad, objf = xent_from_post(post if ok else np.zeros_like(x), y, xr, w, ok, **mut)
    return grad, objf, w * T


# ---------------------------------------------------------------- the GPU test's cases
def _lattice(seed, P, T):
    """chain_ref.ragged_cases' lattice: labels 0 and P + 3 among its skip arcs, finals within
    the first T states."""
    f = cr.lattice(seed, 14, P, 4, max(T, 4))
    f["final_state"] = np.array([0, min(T, 5), 9], np.int32)
    return f


# name -> P, sequences (family, T), layout, pad columns (ldx - P, ldg - P), xr, w, and the index
# of a sequence whose chain objective is made non-finite (+inf on its numerator path), or None.
# P: 8 (one 16-byte access per row), 13 (the scalar path), 200, 3080 and 4096 (two column chunks
# of the kernel's 2048-column LDS row; 4096 is the most pdfs a den graph takes). T: 0, 1, 2, 9.
CASES = {
    "p200_stride3": dict(P=200, seqs=[("chain", 9), ("lattice", 9), ("lattice", 1), ("chain", 2)],
                         compact=False, pad=(24, 8), xr=0.1, w=0.5, bad=None),
    "p200_compact": dict(P=200, seqs=[("lattice", 9), ("chain", 2)], compact=True, pad=(0, 0), xr=0.1, w=1.0, bad=None),
    "p13_bad_zero": dict(P=13, seqs=[("chain", 9), ("chain", 0), ("chain", 9), ("lattice", 2)],
                         compact=True, pad=(0, 0), xr=0.1, w=1.0, bad=2),
    "p13_stride3": dict(P=13, seqs=[("lattice", 9), ("chain", 1)], compact=False, pad=(3, 1), xr=0.1, w=0.5, bad=None),
    "p8": dict(P=8, seqs=[("chain", 9), ("lattice", 2)], compact=False, pad=(8, 16), xr=0.1, w=1.0, bad=None),
    "p8_xr0": dict(P=8, seqs=[("chain", 9), ("lattice", 2)], compact=False, pad=(0, 0), xr=0.0, w=1.0, bad=None),
    "p3080": dict(P=3080, seqs=[("lattice", 2), ("chain", 1)], compact=True, pad=(0, 0), xr=0.1, w=1.0, bad=None),
    "p4096": dict(P=4096, seqs=[("chain", 2), ("lattice", 1)], compact=False, pad=(8, 8), xr=0.1, w=0.5, bad=None),
}


class Case:
    """One case of CASES, built once per process: den graph, FSTs, chain outputs x, xent
    outputs y (fp16), and the float64 reference of every sequence."""

    def __init__(self, name):
        c = CASES[name]
        self.name, self.P, self.xr, self.w = name, c["P"], c["xr"], c["w"]
        self.compact, self.pad, self.bad = c["compact"], c["pad"], c["bad"]
        seed = sum(name.encode())
        self.g = cr.skewed_den(seed, 5, self.P, used=min(self.P, 7))
        self.init = cr.den_init(self.g)
        self.frames = np.array([T for _, T in c["seqs"]], np.int32)
        self.fsts, self.xs, self.ys = [], [], []
        for i, (fam, T) in enumerate(c["seqs"]):
            f = cr.weighted_chain(seed + i, max(2, min(T, 6)), self.P) if fam == "chain" else _lattice(seed + i, self.P, T)
            x = cr.outputs(seed + 50 + i, T, self.P) if T > 0 else np.zeros((0, self.P), np.float16)
            if self.bad == i:
                x[0, f["pdf1"][0] - 1] = np.inf
            self.fsts.append(f)
            self.xs.append(x)
            self.ys.append(xent_outputs(seed + 100 + i, T, self.P) if T > 0 else np.zeros((0, self.P), np.float16))
        self._ref = {}

    def ref(self, i, **mut):
        """(grad, objf, weight) of sequence i; ok is False for the case's bad sequence only."""
        key = (i, tuple(sorted(mut.items())))
        if key not in self._ref:
            self._ref[key] = xent_f64(self.fsts[i], self.xs[i], self.ys[i], self.xr, self.w,
                                      ok=False if self.bad == i else None, **mut)
        return self._ref[key]


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]
