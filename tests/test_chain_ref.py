"""tests/chain_ref.py checked without a GPU: its float64 references against the C oracle on
every case tests/test_gpu_chain_graphs.py uses, the generators' properties, and the
sensitivity of the chosen inputs.

The GPU bars (against float64): numerator log-prob 1e-2, den log-prob 1e-4 per
frame, objective 1e-3 per frame, gradient elements w * 1e-4 + one fp16 ulp, l2_term 1e-3
relative. Condition asserted here: the float32 oracle's distance from float64 is at most a
quarter of each bar on every case, so the float32 reference alone sits far inside the bars
and the float64 references are the oracle's computation (pinned so far only on a weight-0
linear FST and one uniform 24-state graph).

Measured maxima of |oracle - float64| per case group (printed by the first test with -s).
The gradient column is the largest element error, with its share of that element's bar:

  group                           num lp    den lp/frame  objf/frame  gradient
  chain20, lattice40, lattice250  1.2e-05   1.7e-07       4.1e-07     1.0e-05 (3.0 %)
  ragged (T = 1, 2, 7, 8, 9)      4.2e-07   3.9e-07       4.5e-07     1.4e-06 (0.1 %)
  mixed, zero                     9.2e-06   1.5e-07       3.5e-07     1.2e-05 (1.9 %)
  lds:* (S = 300, 301)            1.5e-05   3.3e-07       8.8e-07     1.5e-05 (2.3 %)
  den:s1 .. den:s65               1.9e-05   1.7e-07       1.8e-06     2.4e-05 (15.5 %)
  den:s1000, den:s1000z           1.4e-06   5.7e-07       4.8e-07     2.9e-06 (0.3 %)
  den:s3000                       1.9e-06   1.2e-06       1.1e-06     2.8e-05 (4.3 %)
  gleg:2, 64, 80, 300             8.7e-06   1.9e-07       8.6e-07     8.2e-06 (8.2 %)
  opts (3 option sets)            7.4e-07   2.0e-07       2.8e-07     4.8e-06 (0.3 %)
  life:*                          2.2e-06   8.1e-08       1.1e-07     3.2e-06 (0.3 %)
  quarter of the bar              2.5e-03   2.5e-05       2.5e-04     (25 %)
l2_term (opts, l2 = 5e-4): 8.1e-08 relative, against 2.5e-4.
"""
import numpy as np
import pytest

import chain_ref as cr
import oracle

QUARTER = 0.25


def _distances(b, i, opts):
    x = b.xs[i].astype(np.float32)
    d, r = oracle.chain_objf(b.g, b.init, b.fsts[i], x, **opts)
    d64, r64 = b.ref(i, **opts)
    T = int(b.frames[i])
    w = opts.get("weight", 1.0)
    out = dict(num=abs(r["num_logprob"] - r64["num_logprob"]),
               den=abs(r["den_logprob"] - r64["den_logprob"]) / T,
               objf=abs(r["objf"] - r64["objf"]) / T,
               grad=float(np.max(np.abs(d - d64))),
               grad_share=float(np.max(np.abs(d - d64) / cr.grad_bar(d64, w))))
    assert r["ok"] == r64["ok"] == 1 and r["out_of_range"] == r64["out_of_range"]
    assert r["total_weight"] == r64["total_weight"] and r["frames"] == r64["frames"]
    if opts.get("l2", 0.0) > 0:
        out["l2"] = abs(r["l2_term"] - r64["l2_term"]) / abs(r64["l2_term"])
    else:
        assert r["l2_term"] == r64["l2_term"] == 0.0
    return out


@pytest.mark.parametrize("name,seqs,opts", cr.all_batch_cases(),
                         ids=lambda v: v if isinstance(v, str) else None)
def test_oracle_within_quarter_of_the_gpu_bars(name, seqs, opts):
    b = cr.batch(name)
    worst = {}
    for i in (range(len(b.fsts)) if seqs is None else seqs):
        if b.frames[i] == 0:
            continue
        for k, v in _distances(b, i, opts).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(name, opts, {k: "%.2e" % v for k, v in worst.items()})
    assert worst["num"] <= QUARTER * 1e-2
    assert worst["den"] <= QUARTER * 1e-4
    assert worst["objf"] <= QUARTER * 1e-3
    assert worst["grad_share"] <= QUARTER
    assert worst.get("l2", 0.0) <= QUARTER * 1e-3


@pytest.mark.parametrize("case", list(cr.DEN_CASES))
@pytest.mark.parametrize("leaky", cr.LEAKY)
def test_den_posteriors_against_oracle(case, leaky):
    """The den ABI comparison's reference (fp32 input, sequence 0 of the den batch)."""
    b = cr.batch("den:" + case)
    x = b.xs[0].astype(np.float32)
    lp, post = oracle.den_forward_backward(b.g, b.init, x, leaky)
    lp64, post64 = cr.den_f64(b.g, b.init, x, leaky)
    assert abs(lp - lp64) / x.shape[0] <= QUARTER * 1e-4
    assert np.max(np.abs(post - post64) / cr.grad_bar(post64)) <= QUARTER
    np.testing.assert_allclose(post64.sum(1), 1.0, atol=1e-9)


@pytest.mark.parametrize("kind", ["chain20", "lattice40", "lattice250"])
def test_num_posteriors_against_oracle(kind):
    b = cr.batch(kind)
    x = b.xs[0].astype(np.float32)
    lp, post = oracle.num_forward_backward(b.fsts[0], x)
    lp64, post64 = cr.num_f64(b.fsts[0], x)
    assert abs(lp - lp64) <= QUARTER * 1e-2
    assert np.max(np.abs(post - post64)) <= QUARTER * 1e-4
    np.testing.assert_allclose(post64.sum(1), 1.0, atol=1e-9)


def test_den_f64_matches_dense_restatement():
    """den_f64 is the dense-matrix recursion of test_oracle_chain.py, written over arcs."""
    from test_oracle_chain import small_den
    g = small_den()
    init = oracle.den_initial_probs(g)
    x = np.random.default_rng(1).standard_normal((9, g["P"])) * 2
    x[3, 2] = 40.0
    S = g["S"]
    ex = np.exp(np.clip(x, -30, 30))
    i64 = init.astype(np.float64)
    a, logc = i64 * (1 + 0.1 * i64.sum()), 0.0
    s = i64.sum()
    for t in range(9):
        M = np.zeros((S, S))
        np.add.at(M, (g["src"], g["dst"]), g["tp"].astype(np.float64) * ex[t, g["pdf0"]])
        n = (a @ M) / s
        logc += np.log(s)
        s = n.sum()
        a = n + s * 0.1 * i64
    assert abs(cr.den_f64(g, init, x, 0.1)[0] - (np.log(a.sum()) + logc)) <= 1e-12


# ---------------------------------------------------------------- generator properties
def test_numerator_generators():
    P = cr.DEN65["P"]
    for kind, (f, T) in cr.num_cases(P).items():
        assert cr.final_reachable(f, P), kind
        assert np.isfinite(cr.num_f64(f, cr.outputs(1, T, P), posteriors=False)[0]), kind
    for f, T in cr.ragged_cases(P):
        assert np.isfinite(cr.num_f64(f, cr.outputs(1, T, P), posteriors=False)[0]), T
    f, _ = cr.num_cases(P)["lattice40"]
    S = f["S"]
    src, dst, lab = cr._arc_src(f), f["dst"], f["pdf1"]
    outdeg, indeg = np.bincount(src, minlength=S), np.bincount(dst[src != dst], minlength=S)
    assert outdeg[S - 4] == outdeg[S - 3] == 0 and indeg[S - 4] == indeg[S - 3] == 1   # dead ends
    assert indeg[S - 2] == indeg[S - 1] == 0 and outdeg[S - 2] == outdeg[S - 1] == 2   # unreachable
    assert np.any(lab == 0) and np.any(lab == P + 3)
    assert len(f["final_state"]) == 3 and len(np.unique(f["final_w"])) == 3
    groups = np.bincount(lab[(lab > 0) & (lab <= P)])
    assert groups.max() >= 10            # npdf = 5: groups of tens of arcs
    w = cr.num_cases(P)["chain20"][0]["logw"]
    assert len(np.unique(w)) == len(w) and w.max() <= -0.05 and w.min() >= -3.0


@pytest.mark.parametrize("case", list(cr.LDS_CASES))
def test_sized_gives_the_requested_counts(case):
    c = cr.LDS_CASES[case]
    f = cr.batch("lds:" + case).fsts[1]
    assert cr.num_counts(f) == (c["S"], c["A"], c["G"])
    assert len(f["final_state"]) == c["S"] and f["pdf1"].min() >= 1 and f["pdf1"].max() <= cr.DEN_WIDE["P"]
    words = 4 * c["S"] + 3 * c["G"] + 6 * c["A"] + 6
    assert cr.num_lds_words(f) == words
    # which side of kf_chain_compute's rule each case is on
    assert (words, cr.batch_uses_lds(cr.batch("lds:" + case).fsts)) == {
        "fit": (16384, True), "fit+1arc": (16390, False), "g1024": (13278, True),
        "g1025": (13281, False)}[case]


@pytest.mark.parametrize("case", list(cr.DEN_CASES))
def test_skewed_den_properties(case):
    kw = cr.DEN_CASES[case]
    g = cr.den_graph(case)
    S, P = kw["S"], kw["P"]
    assert (g["S"], g["P"], g["A"]) == (S, P, len(g["src"])) and g["A"] == kw.get("A", g["A"])
    indeg, outdeg = np.bincount(g["dst"], minlength=S), np.bincount(g["src"], minlength=S)
    assert int((indeg == 0).sum()) == kw.get("nosrc", 0)
    assert int((outdeg == 0).sum()) == kw.get("nosink", 0)
    used = np.bincount(g["pdf0"], minlength=P)
    assert int((used == 0).sum()) == P - kw.get("used", P)
    core = S - kw.get("nosrc", 0) - kw.get("nosink", 0)
    assert indeg[0] >= S / 2 or S == 1
    assert len(np.unique(g["src"][g["hub_in"]])) >= core - 1    # an arc from every other core state
    assert len(np.unique(g["dst"][g["src"] == 0])) >= core - 1  # ... and to it
    assert np.all(np.diff(g["src"]) >= 0)                               # listed state by state
    assert np.any(g["tp"] == 0) and np.all(g["tp"] >= 0) and g["tp"].max() <= np.exp(-0.5)
    key = g["src"].astype(np.int64) * S + g["dst"]
    full = (key * P + g["pdf0"]) * 2
    assert len(np.unique(key)) < len(key)                # parallel arcs
    if S > 1:
        assert len(np.unique(full)) < len(full)          # exact duplicates (same src, dst, pdf)
        _, cnt = np.unique(key, return_counts=True)
        assert cnt.max() >= 3                            # ... and a third arc with another pdf
    if kw.get("heavy"):
        assert used.max() >= 0.45 * g["A"]
    init = cr.den_init(g)
    assert abs(float(init.sum()) - 1.0) < 1e-5 and np.all(init > 0)


def _slice_lengths(key, n):
    """SELL-64 slice lengths of a table keyed by `key`: rows sorted by degree, 64 per slice."""
    deg = np.sort(np.bincount(key, minlength=n))[::-1]
    return np.concatenate([deg, np.zeros(-n % 64, int)]).reshape(-1, 64).max(1)


def test_den_tables_get_zero_length_slices():
    """s1000: a slice of length 0 in the by-destination and by-source tables, seven in the
    by-pdf table; s1000z: two in the first two; s3000: a hub slice of thousands of steps beside slices of 8 - 16."""
    g = cr.den_graph("s1000")
    assert int((_slice_lengths(g["dst"], g["S"]) == 0).sum()) == 1
    assert int((_slice_lengths(g["src"], g["S"]) == 0).sum()) == 1
    assert int((_slice_lengths(g["pdf0"], g["P"]) == 0).sum()) == 7
    g = cr.den_graph("s1000z")
    assert int((_slice_lengths(g["dst"], g["S"]) == 0).sum()) == 2
    assert int((_slice_lengths(g["src"], g["S"]) == 0).sum()) == 2
    g = cr.den_graph("s3000")
    ln = _slice_lengths(g["dst"], g["S"])
    assert ln[0] >= 2999 and np.median(ln) <= 24
    assert _slice_lengths(g["pdf0"], g["P"])[0] >= 0.45 * g["A"]


# ---------------------------------------------------------------- sensitivity of the inputs
def _beyond_bars(d_ref, r_ref, d_new, r_new, frames):
    """The change moves a result beyond a GPU bar."""
    return (abs(r_new["num_logprob"] - r_ref["num_logprob"]) > 1e-2 or
            abs(r_new["den_logprob"] - r_ref["den_logprob"]) / frames > 1e-4 or
            bool(np.any(np.abs(d_new - d_ref) > cr.grad_bar(d_ref))))


@pytest.mark.parametrize("kind", ["chain20", "lattice40", "lattice250"])
def test_permuted_in_arc_weights_show(kind):
    """A wrong permutation of in_w (weights rotated inside each state's in-arc list)."""
    b = cr.batch(kind)
    f = dict(b.fsts[0])
    w = f["logw"].copy()
    dst = f["dst"]
    for s in range(f["S"]):
        k = np.flatnonzero(dst == s)
        w[k] = np.roll(f["logw"][k], 1)
    f["logw"] = w
    d0, r0 = b.ref(0)
    d1, r1 = cr.objf_f64(b.g, b.init, f, b.xs[0])
    assert abs(r1["num_logprob"] - r0["num_logprob"]) > 1e-2
    assert np.any(np.abs(d1 - d0) > cr.grad_bar(d0))


@pytest.mark.parametrize("kind", ["lattice40", "lattice250"])
def test_swapped_final_weights_show(kind):
    b = cr.batch(kind)
    f = dict(b.fsts[0])
    f["final_w"] = f["final_w"][[1, 0, 2]]
    d0, r0 = b.ref(0)
    d1, r1 = cr.objf_f64(b.g, b.init, f, b.xs[0])
    assert _beyond_bars(d0, r0, d1, r1, b.frames[0])


@pytest.mark.parametrize("case", [c for c in cr.DEN_CASES if cr.DEN_CASES[c]["S"] >= 63])
@pytest.mark.parametrize("leaky", cr.LEAKY)
def test_dropped_hub_in_arcs_show(case, leaky):
    """The hub's last 8 in-arcs (the tail of the longest slice) dropped."""
    b = cr.batch("den:" + case)
    cut = cr.den_without(b.g, b.g["hub_in"][-8:])
    for i in range(3):
        lp0, p0 = cr.den_f64(b.g, b.init, b.xs[i], leaky)
        lp1, p1 = cr.den_f64(cut, b.init, b.xs[i], leaky)
        assert abs(lp1 - lp0) / b.frames[i] > 1e-4 or np.any(np.abs(p1 - p0) > cr.grad_bar(p0)), i


@pytest.mark.parametrize("case", [c for c in cr.DEN_CASES if "used" in cr.DEN_CASES[c]])
def test_unused_pdf_posterior_moved_shows(case):
    """An unused pdf's zero posterior written one pdf lower (an off-by-one row of the
    pdf-keyed table) moves the gradient beyond its bar."""
    b = cr.batch("den:" + case)
    used = cr.DEN_CASES[case]["used"]
    d0, _ = b.ref(0)
    moved = d0.copy()
    moved[:, used - 1], moved[:, used] = d0[:, used], d0[:, used - 1]
    assert np.all(cr.den_f64(b.g, b.init, b.xs[0])[1][:, used:] == 0)
    assert np.any(np.abs(moved - d0) > cr.grad_bar(d0))
