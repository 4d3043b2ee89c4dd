"""float64 references of the chain objective and the graph families of
tests/test_gpu_chain_graphs.py. No GPU needed: tests/test_chain_ref.py checks the references
against the C oracle (oracle/kf_oracle_chain.c) and the generators' properties from here alone.

References (numpy float64, no code shared with the oracle or the kernels):
  num_f64   log-domain forward-backward of an arbitrary CSR FST (chain_det.cu:55-237): arcs
            whose label is <= 0 or > P are skipped; total over the finals with their weights.
  den_f64   the leaky-HMM recursion of chain_den.cu:496-706 over the arc list (np.add.at), so
            it scales to a few thousand states.
  objf_f64  the assembly of backward.go:224-371: deriv = w * num - w * den, plus the
            out-of-range penalty on even frames (scale 2 * oor, limit +-30), minus
            w * l2 * x; l2_term, total_weight, the out-of-range count and the NaN rule.

Numerator families (dicts in synth.make_num_fst's form, labels 1-based):
  weighted_chain  make_num_fst's topology (self-loop + forward arc) with weights -U[0.05, 3]:
                  a permuted in_w / gw table changes the result.
  lattice         backbone (self-loop + next, valid labels) with 0-2 skip arcs (+2, +3) per
                  state, a share of the skip arcs labelled 0 or P + 3 (skipped), labels from
                  a pool of `npdf` pdfs (groups of many arcs), 3 finals with weights
                  -U[0, 2.5], two reachable dead-end states, two unreachable states.
  sized           chain with skips, every state final, exactly S states, A arcs and G
                  distinct labels: the LDS-layout boundary cases.
Denominator family:
  skewed_den      ring over the core states, a hub (state 0) with an arc to and from every
                  core state, `nosrc` states without in-arcs, `nosink` states without
                  out-arcs, only the first `used` pdfs used, optionally one pdf on half of
                  the arcs, duplicated (src, dst) pairs, exact duplicates, tp = 0 arcs,
                  tp = exp(-U[0.5, 8]).
den_init gives the initial probabilities the den cases use: the 100-iteration rule of
denominator.go:131-171 mixed with 10 % uniform, so that states without in-arcs carry mass
(under the rule alone they would hold zero throughout and their out-arcs never matter).
"""
import numpy as np

NEG = -np.inf


# ---------------------------------------------------------------- references
def _arc_src(f):
    return np.repeat(np.arange(f["S"]), np.diff(np.asarray(f["row_ptr"], np.int64)))


def num_f64(f, x, posteriors=True):
    """(total log-prob, posteriors [T x P]) of FST `f` on outputs x [T x P]."""
    x = np.asarray(x, np.float64)
    T, P = x.shape
    S = int(f["S"])
    src = _arc_src(f)
    dst = np.asarray(f["dst"], np.int64)
    pdf = np.asarray(f["pdf1"], np.int64)
    w = np.asarray(f["logw"], np.float64)
    ok = (pdf > 0) & (pdf <= P)
    src, dst, pdf0, w = src[ok], dst[ok], pdf[ok] - 1, w[ok]
    fs = np.asarray(f["final_state"], np.int64)
    fw = np.asarray(f["final_w"], np.float64)
    alpha = np.full((T + 1, S), NEG)
    alpha[0, int(f.get("start", 0))] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            np.logaddexp.at(alpha[t + 1], dst, alpha[t, src] + x[t, pdf0] + w)
        total = float(np.logaddexp.reduce(alpha[T, fs] + fw)) if len(fs) else NEG
        if not posteriors:
            return total, None
        beta = np.full((T + 1, S), NEG)
        np.logaddexp.at(beta[T], fs, fw)
        post = np.zeros((T, P))
        for t in range(T - 1, -1, -1):
            v = beta[t + 1, dst] + x[t, pdf0] + w
            np.logaddexp.at(beta[t], src, v)
            if np.isfinite(total):
                lp = alpha[t, src] + v - total
                np.add.at(post[t], pdf0, np.exp(np.where(np.isnan(lp), NEG, lp)))
    return total, post


def den_f64(g, init, x, leaky=1e-5, posteriors=True):
    """(log-prob, posteriors [T x P]) of the leaky-HMM denominator on x [T x P]: alpha'
    recursion with per-frame normalisation, then the backward / posterior pass."""
    S, P = int(g["S"]), int(g["P"])
    x = np.asarray(x, np.float64)
    T = x.shape[0]
    src, dst, pdf = (np.asarray(g[k], np.int64) for k in ("src", "dst", "pdf0"))
    tp = np.asarray(g["tp"], np.float64)
    ex = np.exp(np.clip(x, -30, 30))
    init = np.asarray(init, np.float64)
    alphas, sums = [], []
    a = init.copy()
    s = a.sum()
    ad = a + s * leaky * init
    alphas.append(ad)
    sums.append(s)
    logc = 0.0
    for t in range(T):
        a = np.zeros(S)
        np.add.at(a, dst, ad[src] * tp * ex[t, pdf])
        a /= s
        logc += np.log(s)
        s = a.sum()
        ad = a + s * leaky * init
        alphas.append(ad)
        sums.append(s)
    total = ad.sum()
    lp = float(np.log(total) + logc)
    if not posteriors:
        return lp, None
    post = np.zeros((T, P))
    bd = np.full(S, 1.0 / total)
    b = bd + leaky * (init @ bd)
    for t in range(T - 1, -1, -1):
        wv = tp * ex[t, pdf] * b[dst]
        np.add.at(post[t], pdf, alphas[t][src] * wv / sums[t])
        bd = np.zeros(S)
        np.add.at(bd, src, wv)
        bd /= sums[t]
        b = bd + leaky * (init @ bd)
    return lp, post


def objf_f64(g, init, f, x, l2=0.0, oor=0.01, leaky=1e-5, weight=1.0):
    """(deriv [T x P], result dict) of one sequence, the fields of oracle.chain_objf."""
    x = np.asarray(x, np.float64)
    T, P = x.shape
    nl, npost = num_f64(f, x)
    dl, dpost = den_f64(g, init, x, leaky)
    deriv = np.zeros((T, P))
    count = 0
    if oor > 0:
        even = (np.arange(T) % 2 == 0)[:, None]
        lo, hi = even & (x < -30), even & (x > 30)
        deriv[lo] += (-30 - x[lo]) * 2 * oor
        deriv[hi] += (30 - x[hi]) * 2 * oor
        count = int(lo.sum() + hi.sum())
    deriv += weight * npost - weight * dpost
    l2_term = 0.0
    if l2 > 0:
        deriv -= weight * l2 * x
        l2_term = -0.5 * weight * l2 * float(np.sum(x * x))
    objf = weight * (nl - dl)
    ok = 1
    if not np.isfinite(objf):   # backward.go:356-363
        deriv[:] = 0
        objf, l2_term, ok = -10.0 * weight * T, 0.0, 0
    return deriv, dict(objf=objf, l2_term=l2_term, total_weight=weight * T, num_logprob=nl,
                       den_logprob=dl, frames=T, out_of_range=count, ok=ok)


# ---------------------------------------------------------------- numerator families
def _csr(S, arcs, finals, final_w):
    """arcs: (src, dst, pdf1, logw) tuples, any order -> CSR dict, arcs of a state in the
    order given."""
    arcs = sorted(enumerate(arcs), key=lambda e: (e[1][0], e[0]))
    src = np.array([a[0] for _, a in arcs], np.int64)
    row_ptr = np.zeros(S + 1, np.int32)
    np.add.at(row_ptr, src + 1, 1)
    return dict(S=S, A=len(arcs), row_ptr=np.cumsum(row_ptr).astype(np.int32),
                dst=np.array([a[1] for _, a in arcs], np.int32),
                pdf1=np.array([a[2] for _, a in arcs], np.int32),
                logw=np.array([a[3] for _, a in arcs], np.float32),
                final_state=np.asarray(finals, np.int32), final_w=np.asarray(final_w, np.float32),
                start=0)


def weighted_chain(seed, S, P):
    rng = np.random.default_rng(seed)
    arcs = []
    for s in range(S):
        arcs.append((s, s))
        if s + 1 < S:
            arcs.append((s, s + 1))
    pdf = rng.integers(1, P + 1, len(arcs))
    w = -rng.uniform(0.05, 3.0, len(arcs))
    return _csr(S, [(a, b, int(p), float(v)) for (a, b), p, v in zip(arcs, pdf, w)], [S - 1], [0.0])


def lattice(seed, S, P, npdf, T, bad_share=0.3):
    """S >= 12 states: core 0 .. S-5, dead ends S-4 and S-3, unreachable S-2 and S-1. Finals:
    the last core state and two within the first T states (weights -U[0, 2.5]), so the
    total is finite at T frames."""
    rng = np.random.default_rng(seed)
    C = S - 4
    pool = rng.choice(P, size=min(npdf, P), replace=False) + 1
    lab = lambda: int(pool[rng.integers(len(pool))])   # noqa: E731
    wt = lambda: float(-rng.uniform(0.05, 3.0))        # noqa: E731
    arcs = []
    for s in range(C):
        arcs.append((s, s, lab(), wt()))
        if s + 1 < C:
            arcs.append((s, s + 1, lab(), wt()))
        for hop in (2, 3)[:rng.integers(0, 3)]:
            if s + hop < C:
                bad = rng.random() < bad_share
                arcs.append((s, s + hop, (0, P + 3)[rng.integers(2)] if bad else lab(), wt()))
    for k, d in enumerate((S - 4, S - 3)):           # dead ends, entered early (live alpha)
        arcs.append((2 + 3 * k, d, lab(), wt()))
    for u in (S - 2, S - 1):                         # unreachable: out-arcs only
        arcs.append((u, u, lab(), wt()))
        arcs.append((u, int(rng.integers(0, min(C, T))), lab(), wt()))
    hi = min(T, C - 1)
    early = rng.choice(np.arange(hi // 2, hi), size=2, replace=False)
    finals = sorted(int(v) for v in early) + [C - 1]
    return _csr(S, arcs, finals, -rng.uniform(0.0, 2.5, 3))


def sized(seed, S, A, G, P):
    """Exactly S states, A arcs (2S - 1 backbone arcs plus skips s -> s + 2, s + 3, ...), G
    distinct labels in [1, P]; every state final."""
    assert A >= 2 * S - 1 and G <= min(A, P) and S >= 3
    rng = np.random.default_rng(seed)
    pairs = []
    for s in range(S):
        pairs.append((s, s))
        if s + 1 < S:
            pairs.append((s, s + 1))
    hop, s = 2, 0
    while len(pairs) < A:
        if s + hop < S:
            pairs.append((s, s + hop))
        s += 1
        if s + hop >= S:
            s, hop = 0, hop + 1
            assert hop < S, "too many arcs for S states"
    pdfs = rng.choice(P, size=G, replace=False) + 1
    lab = np.concatenate([pdfs, pdfs[rng.integers(0, G, A - G)]])
    rng.shuffle(lab)
    w = -rng.uniform(0.05, 3.0, A)
    return _csr(S, [(a, b, int(p), float(v)) for (a, b), p, v in zip(pairs, lab, w)],
                np.arange(S), -rng.uniform(0.0, 2.5, S))


def num_counts(f, P=None):
    """(S, A, G) as kf_num_batch_create counts them: G = distinct labels > 0."""
    lab = np.asarray(f["pdf1"])
    return int(f["S"]), int(f["A"]), int(len(np.unique(lab[lab > 0])))


def num_lds_words(f):
    """k_num_fb's LDS layout (num_lds_layout): 4S + 3G + 6A + 6 words."""
    S, A, G = num_counts(f)
    return 4 * S + 3 * G + 6 * A + 6


def batch_uses_lds(fsts):
    """kf_chain_compute's rule: the batch runs k_num_fb when the largest layout fits 64 KiB
    and every FST has S, G <= 1024; otherwise k_logfb."""
    return (max(num_lds_words(f) for f in fsts) * 4 <= 64 * 1024 and
            all(num_counts(f)[0] <= 1024 and num_counts(f)[2] <= 1024 for f in fsts))


def final_reachable(f, P):
    """A final state can be reached from the start over arcs with a label in [1, P]."""
    src, dst, lab = _arc_src(f), np.asarray(f["dst"]), np.asarray(f["pdf1"])
    seen = np.zeros(f["S"], bool)
    seen[int(f.get("start", 0))] = True
    ok = (lab > 0) & (lab <= P)
    for _ in range(f["S"]):
        nxt = seen.copy()
        nxt[dst[ok & seen[src]]] = True
        if np.array_equal(nxt, seen):
            break
        seen = nxt
    return bool(seen[np.asarray(f["final_state"])].any())


# ---------------------------------------------------------------- denominator family
def skewed_den(seed, S, P, A=None, nosrc=0, nosink=0, used=None, heavy=False):
    """See the module docstring. Core states 0 .. C-1 (C = S - nosrc - nosink), then the
    `nosrc` states, then the `nosink` states. A: total arcs (default: the mandatory arcs plus
    2 S random core arcs, at least `used`). Returns the dict chain.DenGraph takes, with
    "hub_in" = the hub's in-arc indices (in arc order)."""
    rng = np.random.default_rng(seed)
    used = P if used is None else used
    C = S - nosrc - nosink
    assert C >= 1 and 1 <= used <= P
    src = list(range(C)) + [0] * (C - 1) + list(range(1, C))
    dst = [(s + 1) % C for s in range(C)] + list(range(1, C)) + [0] * (C - 1)
    for u in range(C, C + nosrc):
        src += [u, u]
        dst += [int(v) for v in rng.integers(0, C, 2)]
    for u in range(C + nosrc, S):
        src += [int(v) for v in rng.integers(0, C, 2)]
        dst += [u, u]
    fixed = len(src)
    ndup = min(3, C)
    A = max(fixed + 2 * S, used) + 2 * ndup if A is None else A
    assert A >= max(fixed, used) + 2 * ndup
    nfill = A - fixed - 2 * ndup
    src += [int(v) for v in rng.integers(0, C, nfill)]
    dst += [int(v) for v in rng.integers(0, C, nfill)]
    src, dst = np.array(src, np.int64), np.array(dst, np.int64)
    pdf = rng.integers(0, used, len(src))
    if heavy:
        pdf[rng.random(len(src)) < 0.5] = used // 2
    cover = rng.permutation(len(src))[:used]        # every used pdf has an arc
    pdf[cover] = np.arange(used)
    tp = np.exp(-rng.uniform(0.5, 8.0, len(src)))
    # parallel arcs: the same (src, dst) with another pdf, and exact duplicates
    pick = rng.choice(C, ndup, replace=False)       # ring arcs pick -> pick + 1
    src = np.concatenate([src, src[pick], src[pick]])
    dst = np.concatenate([dst, dst[pick], dst[pick]])
    pdf = np.concatenate([pdf, (pdf[pick] + 1) % used, pdf[pick]])
    tp = np.concatenate([tp, np.exp(-rng.uniform(0.5, 8.0, ndup)), tp[pick]])
    if nfill > 0:                                   # a few dead arcs among the random ones
        tp[fixed + rng.choice(nfill, min(3, nfill), replace=False)] = 0.0
    order = np.argsort(src, kind="stable")
    src, dst, pdf, tp = src[order], dst[order], pdf[order], tp[order]
    return dict(S=S, P=P, A=len(src), src=src.astype(np.int32), dst=dst.astype(np.int32),
                pdf0=pdf.astype(np.int32), tp=tp.astype(np.float32), start=0,
                hub_in=np.flatnonzero(dst == 0))


def den_init(g):
    """0.9 x the 100-iteration rule of denominator.go:131-171 + 0.1 uniform, float32."""
    S = int(g["S"])
    src, dst = np.asarray(g["src"], np.int64), np.asarray(g["dst"], np.int64)
    tp = np.asarray(g["tp"], np.float64)
    cur = np.zeros(S)
    cur[int(g["start"])] = 1.0
    avg = np.zeros(S)
    for _ in range(100):
        avg += cur / 100.0
        nxt = np.zeros(S)
        np.add.at(nxt, dst, cur[src] * tp)
        tot = nxt.sum()
        cur = nxt / tot if tot > 0 else nxt
    return (0.9 * avg + 0.1 / S).astype(np.float32)


def den_without(g, drop):
    """`g` without the arcs whose indices are in `drop`."""
    keep = np.ones(g["A"], bool)
    keep[np.asarray(drop)] = False
    out = {k: (v[keep] if isinstance(v, np.ndarray) and k != "hub_in" else v) for k, v in g.items()}
    out["A"] = int(keep.sum())
    out["hub_in"] = np.flatnonzero(out["dst"] == 0)
    return out


# ---------------------------------------------------------------- inputs and bars
def outputs(seed, T, P, scale=2.5):
    """fp16 outputs: standard_normal * scale, with +40 and -40 planted on an even frame and
    one of each on an odd frame (where T allows), columns fixed by the seed."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, P)) * scale).astype(np.float16)
    c = rng.choice(P, size=min(4, P), replace=False)
    te = 2 if T > 2 else 0
    x[te, c[0]] = 40.0
    x[te, c[1 % len(c)]] = -40.0
    if T > 1:
        to = 3 if T > 3 else 1
        x[to, c[2 % len(c)]] = 40.0
        x[to, c[3 % len(c)]] = -40.0
    return x


def grad_bar(ref, w=1.0):
    """|d| allowed on a gradient element: w * 1e-4 + one fp16 ulp of the value."""
    return w * 1e-4 + np.abs(ref) * 2.0 ** -10


# ---------------------------------------------------------------- the case tables
DEN65 = dict(seed=65, S=65, P=129)                 # the numerator cases' den graph
DEN_WIDE = dict(seed=66, S=65, P=1100)             # labels up to 1025 groups (LDS boundary)

DEN_CASES = {                                       # name -> skewed_den arguments
    "s1": dict(seed=1, S=1, P=3),
    "s5": dict(seed=2, S=5, P=7),
    "s63": dict(seed=3, S=63, P=33, used=20, nosrc=3, nosink=3),
    "s64": dict(seed=4, S=64, P=33, used=20, nosrc=3, nosink=3),
    "s65": dict(seed=5, S=65, P=33, used=20, nosrc=3, nosink=3),
    "s1000": dict(seed=6, S=1000, P=1025, used=600, nosrc=70, nosink=70),
    "s3000": dict(seed=7, S=3000, P=201, A=30000, heavy=True),
    # s1000 leaves one all-zero slice in the by-destination and by-source tables (70 of
    # 1000 rows); 110 rows without arcs leave two
    "s1000z": dict(seed=8, S=1000, P=65, used=40, nosrc=110, nosink=110),
}
DEN_FRAMES = (9, 16, 16)                            # ragged: sequences 0, 1, 2 of a den case
LEAKY = (1e-5, 0.1)

# the largest k_num_fb layout: 4 * 301 + 3 * 100 + 6 * 2479 + 6 = 16384 words = 64 KiB
LDS_CASES = {
    "fit": dict(seed=31, S=301, A=2479, G=100),
    "fit+1arc": dict(seed=31, S=301, A=2480, G=100),
    "g1024": dict(seed=32, S=300, A=1500, G=1024),
    "g1025": dict(seed=32, S=300, A=1500, G=1025),
}


def num_cases(P):
    """name -> (fst, T) of the numerator families on a den graph of P pdfs."""
    return {
        "chain20": (weighted_chain(11, 20, P), 24),
        "lattice40": (lattice(12, 40, P, 5, 24), 24),
        "lattice250": (lattice(13, 250, P, 30, 40), 40),
    }


def ragged_cases(P):
    """T = 1, 2, 7, 8, 9 (NUM_POST_FR = 8, POST_FRAMES = 2, k_num_fb's frame-parity double
    buffer): lattices whose early finals lie within the first T states."""
    out = []
    for i, T in enumerate((1, 2, 7, 8, 9)):
        f = lattice(40 + i, 14, P, 4, max(T, 4))
        f["final_state"] = np.array([0, min(T, 5), 9], np.int32)  # state 0: final at any T
        out.append((f, T))
    return out


# ---------------------------------------------------------------- batches (CPU and GPU tests)
def layout(frames, stride=3, lead=2, compact=False):
    """(row0, rows): sequence i, frame t at row row0[i] + t * stride. Default: `lead`
    unsupervised rows before every sequence and one after; compact: stride 1, row0[i] = the
    frames before it (the bench's compact-row layout)."""
    row0, r = [], 0
    for T in frames:
        if compact:
            row0.append(r)
            r += T
        else:
            row0.append(r + lead)
            r += lead + max(T, 1) * stride + 1
    return np.array(row0, np.int32), r


PAD = 9.0        # pad columns of the output buffer (ld > P)
SENTINEL = 7.0   # gradient buffer before a compute


def place(xs, row0, stride, rows, P, ld=None, seed=0):
    """The [rows x ld] fp16 output buffer: the sequences' frames at their rows, random
    values on every other row, PAD in the columns past P."""
    ld = P if ld is None else ld
    big = (np.random.default_rng(seed).standard_normal((rows, ld)) * 2).astype(np.float16)
    big[:, P:] = PAD
    for x, r0 in zip(xs, row0):
        big[r0 + np.arange(x.shape[0]) * stride, :P] = x
    return big


class Batch:
    """One minibatch of a test: den graph, initial probabilities, numerator FSTs, frame
    counts and the sequences' fp16 outputs; ref() caches the float64 results."""

    def __init__(self, name, den, seqs):
        self.name = name
        self.g = skewed_den(**den) if "seed" in den else den
        self.init = den_init(self.g)
        self.P = self.g["P"]
        self.fsts = [s[0] for s in seqs]
        self.frames = np.array([s[1] for s in seqs], np.int32)
        self.xs = [outputs(s[2], s[1], self.P) if s[1] > 0 else np.zeros((0, self.P), np.float16)
                   for s in seqs]
        self._ref = {}

    def ref(self, i, l2=0.0, oor=0.01, leaky=1e-5, weight=1.0):
        key = (i, l2, oor, leaky, weight)
        if key not in self._ref:
            self._ref[key] = objf_f64(self.g, self.init, self.fsts[i], self.xs[i], l2, oor, leaky, weight)
        return self._ref[key]


_dens, _batches = {}, {}


def den_graph(name):
    """The named den graph (DEN_CASES, "den65", "wide"), built once."""
    if name not in _dens:
        kw = dict(den65=DEN65, wide=DEN_WIDE).get(name) or DEN_CASES[name]
        _dens[name] = skewed_den(**kw)
    return _dens[name]


G_LEG_NSEQ = {4: 2, 2: 80, 1: 300}   # sequences that give den_pick_G = 4, 2, 1 on 256 CUs
LOCAL_NSEQ = 64                      # ... and G = 4 with every unit's workgroups on one XCD
OPTS = {                              # the option sets of the options-and-layout test
    "default": dict(),
    "l2": dict(l2=5e-4, oor=0.0, leaky=0.05, weight=0.5),
    "w2": dict(weight=2.0, oor=0.05),
}


def g_leg_sample(nseq):
    """first, last and a ragged pair (sequences 2, 3 where they exist)."""
    return sorted(set(i for i in (0, 1, 2, 3, nseq - 2, nseq - 1) if 0 <= i < nseq))


def batch(name):
    """The named batch, built once per process:
    chain20 / lattice40 / lattice250   one sequence each            (den65)
    ragged   T = 1, 2, 7, 8, 9                                      (den65)
    mixed    5 sequences from all families                          (den65)
    zero     a zero-frame sequence between two live ones            (den65)
    lds:<LDS_CASES key>   a small companion + the sized FST         (wide)
    den:<DEN_CASES key>   3 short weighted chains, T = 9, 16, 16    (that graph)
    gleg:<nseq>           nseq chains of 12 frames, sequence 3 of 7 (den65)
    opts     3 sequences                                            (den65)
    life:<a|small|large|b>  3 sequences, the same outputs, different FSTs (den65)"""
    if name in _batches:
        return _batches[name]
    kind, _, arg = name.partition(":")
    P65 = DEN65["P"]
    if kind in ("chain20", "lattice40", "lattice250"):
        f, T = num_cases(P65)[kind]
        b = Batch(name, den_graph("den65"), [(f, T, 200 + len(kind))])
    elif kind == "ragged":
        b = Batch(name, den_graph("den65"), [(f, T, 210 + i) for i, (f, T) in enumerate(ragged_cases(P65))])
    elif kind == "mixed":
        b = Batch(name, den_graph("den65"), [
            (weighted_chain(21, 20, P65), 24, 220), (lattice(22, 40, P65, 5, 24), 24, 221),
            (lattice(23, 250, P65, 30, 40), 40, 222), (sized(24, 30, 80, 20, P65), 11, 223),
            (weighted_chain(25, 8, P65), 12, 224)])
    elif kind == "zero":
        b = Batch(name, den_graph("den65"), [
            (weighted_chain(26, 10, P65), 12, 230), (weighted_chain(27, 10, P65), 0, 231),
            (lattice(28, 40, P65, 5, 24), 24, 232)])
    elif kind == "lds":
        P = DEN_WIDE["P"]
        c = LDS_CASES[arg]
        b = Batch(name, den_graph("wide"), [
            (weighted_chain(33, 10, P), 12, 240),
            (sized(c["seed"], c["S"], c["A"], c["G"], P), 12, 241)])
    elif kind == "den":
        g = den_graph(arg)
        b = Batch(name, g, [(weighted_chain(50 + i, 6, g["P"]), T, 250 + i) for i, T in enumerate(DEN_FRAMES)])
    elif kind == "gleg":
        n = int(arg)
        b = Batch(name, den_graph("den65"), [
            (weighted_chain(100 + i, 6, P65), 7 if i == 3 else 12, 1000 + i) for i in range(n)])
    elif kind == "opts":
        b = Batch(name, den_graph("den65"), [
            (weighted_chain(61, 12, P65), 16, 260), (lattice(62, 40, P65, 5, 24), 24, 261),
            (weighted_chain(63, 6, P65), 9, 262)])
    elif kind == "life":
        fs = dict(a=lambda i: weighted_chain(70 + i, 12, P65), small=lambda i: weighted_chain(73 + i, 5, P65),
                  large=lambda i: lattice(76 + i, 60, P65, 8, 12), b=lambda i: weighted_chain(79 + i, 12, P65))[arg]
        b = Batch(name, den_graph("den65"), [(fs(i), 12, 270 + i) for i in range(3)])
    else:
        raise KeyError(name)
    _batches[name] = b
    return b


def all_batch_cases():
    """(batch name, sequence, option dict) of every float64 reference the GPU tests use."""
    out = []
    for n in ("chain20", "lattice40", "lattice250", "ragged", "mixed", "zero"):
        out.append((n, None, {}))
    out += [("lds:" + k, None, {}) for k in LDS_CASES]
    out += [("den:" + k, None, dict(leaky=lk)) for k in DEN_CASES for lk in LEAKY]
    out += [("gleg:%d" % n, g_leg_sample(n), {}) for n in G_LEG_NSEQ.values()]
    out.append(("gleg:%d" % LOCAL_NSEQ, None, {}))
    out += [("opts", None, o) for o in OPTS.values()]
    out += [("life:" + k, None, {}) for k in ("a", "small", "large", "b")]
    return out
