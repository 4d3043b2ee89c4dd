"""kf_chain_compute_weighted: the per-sequence weight and the per-frame deriv
weights of Kaldi egs inside the objective's kernels (k_den_post's gradient assembly,
k_chain_xent), against the unweighted run and the float64 references of tests/chain_ref.py and
tests/xent_ref.py.

The batch: synth.make_den_graph(300 states, 3000 arcs, P pdfs), 3 sequences (the den recursion
sees a pair and a single) of 9, 4 and 1 frames (k_den_post handles two frames per block: a
half-empty last pair, weights that differ inside a pair), stride 3 with lead rows and stride 1
compact, +-40 planted on an even and an odd frame of every sequence (chain_ref.outputs),
l2_regularize > 0, xent_regularize 0.1. P = 200 (the vector path of k_chain_xent) and 203.

Bars: exact scaling by powers of two is exact down to fp16's subnormal range (|g f| >= 2^-14),
one subnormal quantum 2^-24 below it. General weights against float64: test_gpu_chain.py's
1e-4 + one fp16 ulp of the value on every gradient element, its 1e-2 / 1e-4 per frame / 1e-3
per frame on the log-probs and the objective, l2_term 1e-3 relative and total_weight exact
(test_gpu_chain_graphs.py); the xent gradient within chain_ref.grad_bar(ref, w_i * xr) and its
objective within 1e-3 per frame (test_gpu_chain_xent.py).
"""
import numpy as np
import pytest
import torch  # noqa: F401  (the HIP runtime first: the libraries then bind the same copy)

import chain_ref as cr
import xent_ref as xr_

pytestmark = pytest.mark.gpu

FRAMES = np.array([9, 4, 1], np.int32)
L2, OOR, LEAKY, XR = 5e-4, 0.01, 1e-5, 0.1
POW2 = np.array([0.0, 0.25, 0.5, 1.0], np.float32)


class _Case:
    """Den graph, numerator FSTs, fp16 chain outputs and xent outputs of one P."""

    def __init__(self, P):
        from kfp16 import synth
        self.P = P
        self.g = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=P)
        self.init = cr.den_init(self.g)
        # a lattice with out-of-range labels, two weighted chains whose final is reachable
        self.fsts = [xr_._lattice(301, P, 9), cr.weighted_chain(302, 4, P), cr.weighted_chain(303, 2, P)]
        self.xs = [cr.outputs(310 + i, int(T), P) for i, T in enumerate(FRAMES)]
        self.ys = [xr_.xent_outputs(320 + i, int(T), P) for i, T in enumerate(FRAMES)]


_cases = {}


def _case(P):
    if P not in _cases:
        _cases[P] = _Case(P)
    return _cases[P]


def _opts(sw=1.0, xr=XR):
    from kfp16 import chain
    return chain.KfChainOpts(L2, OOR, LEAKY, xr, sw)


class _Run:
    """One Chain over the case's batch in one layout; run() = compute (+ xent) into fresh
    sentinel buffers. seqs: the case's sequences this batch is made of (default: all three, in
    order); chain: a (DenGraph, Chain) to compute with instead of a new pair (it is not closed)."""

    def __init__(self, gpu, c, stride, xs=None, seqs=(0, 1, 2), chain=None):
        from kfp16 import chain as kc
        self.gpu, self.c, self.stride = gpu, c, stride
        self.frames = FRAMES[list(seqs)]
        self.row0, self.rows = cr.layout(self.frames, stride, compact=stride == 1)
        self.own = chain is None
        self.dg = kc.DenGraph(c.g, c.init) if self.own else chain[0]
        self.ch = kc.Chain(self.dg, max_seqs=3, max_frames=int(FRAMES.max())) if self.own else chain[1]
        self.nb = kc.NumBatch([c.fsts[i] for i in seqs])
        self.dx = gpu.upload_fp16(cr.place([(xs or c.xs)[i] for i in seqs], self.row0, stride, self.rows, c.P))
        self.dy = gpu.upload_fp16(cr.place([c.ys[i] for i in seqs], self.row0, stride, self.rows, c.P, seed=1))
        self.sup = np.zeros(self.rows, bool)
        for i in range(len(self.frames)):
            self.sup[self.seq_rows(i)] = True

    def seq_rows(self, i):
        return self.row0[i] + np.arange(self.frames[i]) * self.stride

    def frame_rows(self):
        """row of every (sequence, frame), sequence after sequence: the order of frame_weight"""
        return np.concatenate([self.seq_rows(i) for i in range(len(self.frames))])

    def run(self, opts=None, seq_weight=None, frame_weight=None, xent=True, weighted_call=None):
        gpu, c, P = self.gpu, self.c, self.c.P
        opts = opts or _opts()
        og = gpu.upload_fp16(np.full((self.rows, P), cr.SENTINEL, np.float16))
        kw = {}
        if weighted_call or seq_weight is not None or frame_weight is not None:
            kw = dict(seq_weight=seq_weight, frame_weight=frame_weight)
        self.ch.compute(self.nb, self.dx.ptr, P, self.rows, self.row0, self.frames, self.stride, og.ptr, P, opts, **kw)
        out = dict(res=self.ch.result())
        out["stats"] = self.ch.seq_stats(len(self.frames)).copy()
        out["grad"] = gpu.read_fp16(og.ptr, (self.rows, P))
        if xent:
            xg = gpu.upload_fp16(np.full((self.rows, P), cr.SENTINEL, np.float16))
            self.ch.xent(self.nb, self.dy.ptr, P, xg.ptr, P, opts)
            out["xres"] = self.ch.xent_result()
            out["xgrad"] = gpu.read_fp16(xg.ptr, (self.rows, P))
        return out

    def close(self):
        for h in (self.ch, self.nb, self.dg) if self.own else (self.nb,):
            h.close()


def _res_tuple(r):
    return (r.objf, r.l2_term, r.total_weight, r.num_logprob, r.den_logprob, r.frames, r.out_of_range,
            r.num_ok, r.num_seqs)


def _same(a, b, keys=("grad", "xgrad")):
    for k in keys:
        np.testing.assert_array_equal(a[k].view(np.uint16), b[k].view(np.uint16), err_msg=k)
    np.testing.assert_array_equal(a["stats"].view(np.uint32), b["stats"].view(np.uint32))
    assert _res_tuple(a["res"]) == _res_tuple(b["res"])
    if "xres" in a:
        assert a["xres"] == b["xres"]


def _pow2_weights(seed):
    """weights from {0, 0.25, 0.5, 1} that differ inside every frame pair and hold a zero"""
    rng = np.random.default_rng(seed)
    n = int(FRAMES.sum())
    fw = POW2[rng.integers(0, 4, n)]
    o = 0
    for T in FRAMES:
        for t in range(0, T - 1, 2):
            if fw[o + t] == fw[o + t + 1]:
                fw[o + t + 1] = POW2[(int(np.flatnonzero(POW2 == fw[o + t])[0]) + 1) % 4]
        o += T
    fw[2] = 0.0
    fw[3] = 1.0
    return fw


@pytest.mark.parametrize("stride", [3, 1])
def test_neutral_weights_are_bit_identical(gpu, stride):
    """NULL / NULL through the weighted entry, and all-ones arrays: every output and statistic of
    the compute and of the xent after it as Chain.compute without weights gives them."""
    r = _Run(gpu, _case(200), stride)
    base = r.run()
    assert base["res"].num_ok == 3 and base["res"].out_of_range >= 2 and base["res"].l2_term < 0
    _same(r.run(weighted_call=True), base)
    ones_s, ones_f = np.ones(3, np.float32), np.ones(int(FRAMES.sum()), np.float32)
    _same(r.run(seq_weight=ones_s, frame_weight=ones_f), base)
    _same(r.run(seq_weight=ones_s), base)
    _same(r.run(frame_weight=ones_f), base)
    _same(r.run(), base)           # and an unweighted compute after weighted ones
    r.close()


@pytest.mark.parametrize("stride", [3, 1])
def test_frame_weights_scale_rows_exactly(gpu, stride):
    """Powers of two commute with the fp16 rounding outside the subnormal range: every element
    is the unweighted fp16 value times f; no statistic moves."""
    r = _Run(gpu, _case(200), stride)
    base = r.run()
    fw = _pow2_weights(5)
    got = r.run(seq_weight=np.ones(3, np.float32), frame_weight=fw)
    f_row = np.ones(r.rows, np.float32)
    f_row[r.frame_rows()] = fw
    for k in ("grad", "xgrad"):
        want = base[k].astype(np.float32) * f_row[:, None]
        g = got[k].astype(np.float32)
        normal = np.abs(want) >= 2.0 ** -14
        assert np.any(normal[r.sup]) and np.any(g[r.sup] != base[k].astype(np.float32)[r.sup]), k
        np.testing.assert_array_equal(g[normal], want[normal], err_msg=k)
        assert np.all(np.abs(g - want)[~normal] <= 2.0 ** -24), k
        assert np.all(g[f_row == 0.0] == 0.0), k
        assert np.all(got[k][~r.sup] == cr.SENTINEL), k
    _same(got, base, keys=())      # statistics, result and the xent objective: bit-identical
    r.close()


@pytest.mark.parametrize("P,stride", [(200, 3), (203, 1), (203, 3)])
def test_general_weights_against_float64(gpu, P, stride):
    """A Kaldi-style ramp of deriv weights and per-sequence weights (1, 0.5, 2) on top of
    supervision_weight 0.5, against chain_ref / xent_ref with weight = w_i, times f."""
    c = _case(P)
    r = _Run(gpu, c, stride)
    sw = 0.5
    seq_w = np.array([1.0, 0.5, 2.0], np.float32)
    fws = [np.linspace(0.1, 1.0, int(T)).astype(np.float32) for T in FRAMES]
    got = r.run(opts=_opts(sw), seq_weight=seq_w, frame_weight=np.concatenate(fws))
    grad, xgrad, stats = got["grad"].astype(np.float64), got["xgrad"].astype(np.float64), got["stats"]
    objf = l2 = xobjf = tw = 0.0
    oor = 0
    for i, T in enumerate(FRAMES):
        w = float(np.float32(sw) * seq_w[i])
        f = fws[i].astype(np.float64)[:, None]
        d64, ref = cr.objf_f64(c.g, c.init, c.fsts[i], c.xs[i], L2, OOR, LEAKY, w)
        rows = r.seq_rows(i)
        want = -d64 * f
        err = np.abs(grad[rows] - want) - (1e-4 + np.abs(want) * 2.0 ** -10)
        print("P %d stride %d seq %d: chain gradient max |d| %.2e" % (P, stride, i, np.abs(grad[rows] - want).max()))
        assert np.all(err <= 0), (i, float(err.max()))
        assert abs(stats[i, 0] - ref["num_logprob"]) <= 1e-2
        assert abs(stats[i, 1] - ref["den_logprob"]) / T <= 1e-4
        assert abs(stats[i, 2] - ref["objf"]) / T <= 1e-3
        assert abs(stats[i, 3] - ref["l2_term"]) <= 1e-3 * abs(ref["l2_term"])
        assert stats[i, 4] == np.float32(w) * np.float32(T) and stats[i, 5] == T
        assert int(stats[i, 6]) == ref["out_of_range"] and stats[i, 7] == 1.0
        xg64, xo, xw = xr_.xent_f64(c.fsts[i], c.xs[i], c.ys[i], XR, w)
        xwant = xg64 * f
        xd = np.abs(xgrad[rows] - xwant)
        print("P %d stride %d seq %d: xent gradient max |d| %.2e" % (P, stride, i, xd.max()))
        assert np.all(xd <= cr.grad_bar(xwant, w * XR)), (i, float(xd.max()))
        objf, l2, xobjf, tw, oor = objf + ref["objf"], l2 + ref["l2_term"], xobjf + xo, tw + w * T, oor + ref["out_of_range"]
    n = int(FRAMES.sum())
    res = got["res"]
    assert res.num_ok == 3 and res.frames == n and res.out_of_range == oor
    assert abs(res.objf - objf) / n <= 1e-3
    assert abs(res.l2_term - l2) <= 1e-3 * abs(l2)
    assert res.total_weight == tw                      # sum_i w_i T_i, exact in fp32 here
    assert abs(got["xres"][0] - xobjf) / n <= 1e-3 and got["xres"][1] == tw
    assert np.all(got["grad"][~r.sup] == cr.SENTINEL) and np.all(got["xgrad"][~r.sup] == cr.SENTINEL)
    r.close()


def test_zero_sequence_weight(gpu):
    """seq_weight 0 is legal: a zero objective, and a zero gradient apart from the penalty."""
    c = _case(200)
    r = _Run(gpu, c, 3)
    got = r.run(seq_weight=np.array([1.0, 0.0, 1.0], np.float32))
    base = r.run()
    rows = r.seq_rows(1)
    x = cr.place(c.xs, r.row0, 3, r.rows, c.P)[rows].astype(np.float32)
    pen = np.zeros_like(x)
    even = (np.arange(len(rows)) % 2 == 0)[:, None]
    pen[even & (x < -30)] = ((-30 - x) * 2 * OOR)[even & (x < -30)]
    pen[even & (x > 30)] = ((30 - x) * 2 * OOR)[even & (x > 30)]
    assert np.any(pen)
    np.testing.assert_array_equal(got["grad"][rows].astype(np.float32), (-pen).astype(np.float16).astype(np.float32))
    assert not np.any(got["xgrad"][rows])
    assert got["stats"][1, 2] == 0.0 and got["stats"][1, 3] == 0.0 and got["stats"][1, 4] == 0.0
    for i in (0, 2):
        np.testing.assert_array_equal(got["grad"][r.seq_rows(i)], base["grad"][r.seq_rows(i)])
        np.testing.assert_array_equal(got["stats"][i], base["stats"][i])
    r.close()


def test_not_finite_rule_with_weights(gpu):
    """+inf on the numerator path of sequence 1: zero rows and -10 w_i T for it, the other
    sequences as without the +inf (test_batched_objective_nan_rule, with weights on)."""
    c = _case(200)
    xs = [x.copy() for x in c.xs]
    xs[1][0, c.fsts[1]["pdf1"][0] - 1] = np.inf
    seq_w = np.array([1.0, 0.5, 2.0], np.float32)
    fw = np.linspace(0.25, 1.0, int(FRAMES.sum())).astype(np.float32)
    bad, good = _Run(gpu, c, 3, xs=xs), _Run(gpu, c, 3)
    a = bad.run(seq_weight=seq_w, frame_weight=fw)
    b = good.run(seq_weight=seq_w, frame_weight=fw)
    rows = bad.seq_rows(1)
    assert not np.any(a["grad"][rows]) and not np.any(a["xgrad"][rows])
    assert a["res"].num_ok == 2
    assert a["stats"][1, 7] == 0.0 and a["stats"][1, 2] == -10.0 * 0.5 * FRAMES[1]
    assert a["stats"][1, 4] == 0.5 * FRAMES[1]
    for i in (0, 2):
        for k in ("grad", "xgrad"):
            np.testing.assert_array_equal(a[k][bad.seq_rows(i)], b[k][good.seq_rows(i)])
            assert np.any(a[k][bad.seq_rows(i)])
        np.testing.assert_array_equal(a["stats"][i], b["stats"][i])
    bad.close()
    good.close()


def test_weight_errors_launch_nothing(gpu):
    """A negative weight, a NaN weight, an infinite weight, a wrong count, and xent after a
    weighted compute with another batch: an error that names the place; nothing is written."""
    from kfp16 import KfError, chain
    c = _case(200)
    r = _Run(gpu, c, 3)
    P, n = c.P, int(FRAMES.sum())
    og = gpu.upload_fp16(np.full((r.rows, P), cr.SENTINEL, np.float16))
    xg = gpu.upload_fp16(np.full((r.rows, P), cr.SENTINEL, np.float16))

    def compute(**kw):
        r.ch.compute(r.nb, r.dx.ptr, P, r.rows, r.row0, FRAMES, 3, og.ptr, P, _opts(), **kw)

    fw = np.ones(n, np.float32)
    fw[9 + 2] = -0.5                                     # sequence 1, frame 2
    with pytest.raises(KfError, match="sequence 1, frame 2"):
        compute(frame_weight=fw)
    fw[9 + 2] = 1.0
    fw[n - 1] = np.nan                                   # sequence 2, frame 0
    with pytest.raises(KfError, match="sequence 2, frame 0"):
        compute(frame_weight=fw)
    with pytest.raises(KfError, match="sequence 0:"):
        compute(seq_weight=np.array([np.inf, 1, 1], np.float32))
    with pytest.raises(KfError, match="sequence 2:"):
        compute(seq_weight=np.array([1, 1, -1], np.float32))
    with pytest.raises(KfError, match="frame weights"):
        compute(frame_weight=np.ones(n - 1, np.float32))
    gpu.sync()
    assert np.all(gpu.read_fp16(og.ptr, (r.rows, P)) == cr.SENTINEL)
    compute(seq_weight=np.ones(3, np.float32), frame_weight=np.ones(n, np.float32))
    other = chain.NumBatch(c.fsts)
    with pytest.raises(KfError, match="not the one of the last kf_chain_compute"):
        r.ch.xent(other, r.dy.ptr, P, xg.ptr, P, _opts())
    gpu.sync()
    assert np.all(gpu.read_fp16(xg.ptr, (r.rows, P)) == cr.SENTINEL)
    r.ch.xent(r.nb, r.dy.ptr, P, xg.ptr, P, _opts())     # and the call it refused still works
    assert r.ch.xent_result()[1] == float(n)
    other.close()
    r.close()


def test_weights_are_not_cached_and_replay(gpu):
    """Two weighted computes with one layout and other frame weights: the second one's weights
    are used (the layout cache does not cover them); the same weighted call twice replays bit
    for bit."""
    r = _Run(gpu, _case(200), 3)
    seq_w = np.array([1.0, 0.5, 2.0], np.float32)
    fa, fb = _pow2_weights(7), _pow2_weights(8)
    fb[0] = 0.5 if fa[0] != 0.5 else 0.25
    a1 = r.run(seq_weight=seq_w, frame_weight=fa)
    b = r.run(seq_weight=seq_w, frame_weight=fb)
    a2 = r.run(seq_weight=seq_w, frame_weight=fa)
    _same(a1, a2)
    fresh = _Run(gpu, _case(200), 3)
    _same(fresh.run(seq_weight=seq_w, frame_weight=fb), b)
    row = r.seq_rows(0)[0]
    for k in ("grad", "xgrad"):
        assert np.any(a1[k][row] != b[k][row]), k
    fresh.close()
    r.close()
