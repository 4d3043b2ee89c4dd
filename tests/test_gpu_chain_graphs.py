"""The product chain objective (kf_chain_compute: k_num_fb / k_num_post / k_logfb, k_den_fb,
k_den_post) on weighted numerator FSTs and skewed den graphs, against the float64 references
of tests/chain_ref.py (pinned to the C oracle, without a GPU, by tests/test_chain_ref.py).

Bars (as in test_gpu_chain.py), against float64: numerator log-prob |d| <= 1e-2,
den log-prob <= 1e-4 per frame, objective <= 1e-3 per frame, every gradient element
|d| <= w * 1e-4 + one fp16 ulp of the value (w: the supervision weight), rows without
supervision and pad columns keep their sentinel, out_of_range exact, l2_term 1e-3 relative,
total_weight and frames exact. Every input is fp16, T <= 40.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # the HIP runtime first: the libraries then bind the same copy

import chain_ref as cr

pytestmark = pytest.mark.gpu

WORST = {}   # family -> largest gradient error as a share of its bar (printed per test)


class Dens:
    """Device den graphs, built once per module (the host-side SELL build of the hub graphs
    is the longest part of these tests)."""

    def __init__(self):
        self.g = {}

    def get(self, name):
        from kfp16 import chain
        if name not in self.g:
            g = cr.den_graph(name)
            self.g[name] = chain.DenGraph(g, cr.den_init(g))
        return self.g[name]


@pytest.fixture(scope="module")
def dens(gpu):
    d = Dens()
    yield d
    for v in d.g.values():
        v.close()


def _opts(l2=0.0, oor=0.01, leaky=1e-5, weight=1.0):
    from kfp16 import chain
    return chain.KfChainOpts(l2, oor, leaky, 0.0, weight)


def run(gpu, ch, nb, b, o=None, stride=3, compact=False, pad=(0, 0), seqs=None):
    """One kf_chain_compute of batch `b` (sequences `seqs`, default all). Returns
    (KfChainResult, stats [n x 8], gradient buffer [rows x ldg] fp16, row0, stride)."""
    o = o or {}
    idx = list(range(len(b.fsts))) if seqs is None else list(seqs)
    frames = b.frames[idx]
    stride = 1 if compact else stride
    row0, rows = cr.layout(frames, stride, compact=compact)
    P, ld, ldg = b.P, b.P + pad[0], b.P + pad[1]
    x = cr.place([b.xs[i] for i in idx], row0, stride, rows, P, ld)
    dx = gpu.upload_fp16(x)
    og = gpu.upload_fp16(np.full((rows, ldg), cr.SENTINEL, np.float16))
    ch.compute(nb, dx.ptr, ld, rows, row0, frames, stride, og.ptr, ldg, _opts(**o))
    res = ch.result()
    stats = ch.seq_stats(len(idx)).astype(np.float64)
    got = gpu.read_fp16(og.ptr, (rows, ldg))
    return res, stats, got, row0, stride


def check(b, out, o=None, seqs=None, sample=None, family=None):
    """Every sequence of a run (or the `sample` positions) against float64, and the
    result's totals."""
    o = o or {}
    res, stats, got, row0, stride = out
    idx = list(range(len(b.fsts))) if seqs is None else list(seqs)
    w = o.get("weight", 1.0)
    P = b.P
    sup = np.zeros(got.shape[0], bool)
    worst = 0.0
    for k, i in enumerate(idx):
        T = int(b.frames[i])
        rows = row0[k] + np.arange(T) * stride
        sup[rows] = True
        if T == 0 or (sample is not None and k not in sample):
            continue
        d64, r = b.ref(i, **o)
        s = stats[k]
        print("%s seq %d: num %.2e den/T %.2e objf/T %.2e" % (
            b.name, i, abs(s[0] - r["num_logprob"]), abs(s[1] - r["den_logprob"]) / T, abs(s[2] - r["objf"]) / T))
        assert abs(s[0] - r["num_logprob"]) <= 1e-2, (i, s[0], r["num_logprob"])
        assert abs(s[1] - r["den_logprob"]) / T <= 1e-4, (i, s[1], r["den_logprob"])
        assert abs(s[2] - r["objf"]) / T <= 1e-3, (i, s[2], r["objf"])
        assert int(s[6]) == r["out_of_range"] and s[7] == 1.0, (i, s[6], r["out_of_range"])
        assert s[4] == float(np.float32(w)) * T and s[5] == T
        if o.get("l2", 0.0) > 0:
            assert abs(s[3] - r["l2_term"]) <= 1e-3 * abs(r["l2_term"]), (i, s[3], r["l2_term"])
        else:
            assert s[3] == 0.0
        ref = -d64
        share = np.abs(got[rows, :P].astype(np.float64) - ref) / cr.grad_bar(ref, w)
        worst = max(worst, float(share.max()))
        print("%s seq %d: gradient %.3f of its bar (|d| %.2e)" % (
            b.name, i, share.max(), np.abs(got[rows, :P].astype(np.float64) - ref).max()))
        assert share.max() <= 1.0, (i, float(share.max()), np.unravel_index(share.argmax(), share.shape))
    assert np.all(got[~sup] == cr.SENTINEL)            # rows without supervision
    assert np.all(got[:, P:] == cr.SENTINEL)           # pad columns of the gradient buffer
    live = [i for i in idx if b.frames[i] > 0]
    assert res.num_seqs == len(idx) and res.frames == int(b.frames[idx].sum())
    assert res.num_ok == len(live)
    assert res.total_weight == float(np.float32(w)) * res.frames
    if sample is None:
        refs = [b.ref(i, **o)[1] for i in live]
        assert res.out_of_range == sum(r["out_of_range"] for r in refs)
        assert abs(res.objf - sum(r["objf"] for r in refs)) / res.frames <= 1e-3
        l2 = sum(r["l2_term"] for r in refs)
        assert abs(res.l2_term - l2) <= 1e-3 * abs(l2)
    if family:
        WORST[family] = max(WORST.get(family, 0.0), worst)
        print("family %s: largest gradient error so far %.3f of its bar" % (family, WORST[family]))


def compute_batch(gpu, dens, den_name, b, o=None, **kw):
    from kfp16 import chain
    ch = chain.Chain(dens.get(den_name), max_seqs=len(b.fsts), max_frames=int(max(b.frames.max(), 1)))
    nb = chain.NumBatch(b.fsts)
    out = run(gpu, ch, nb, b, o, **kw)
    return ch, nb, out


# ---------------------------------------------------------------- numerator families
@pytest.mark.parametrize("name", ["chain20", "lattice40", "lattice250", "ragged", "mixed"])
def test_numerator_families(gpu, dens, name):
    """Weighted chains (a permuted in_w / gw shows), lattices (pdf groups of tens of arcs,
    3 weighted finals, labels 0 and P + 3, dead-end and unreachable states), frame counts
    around NUM_POST_FR = 8 / POST_FRAMES = 2 / the xg double buffer's parity, a mixed batch."""
    b = cr.batch(name)
    assert cr.batch_uses_lds(b.fsts)
    _, _, out = compute_batch(gpu, dens, "den65", b)
    check(b, out, family="num:" + name)


def test_zero_frame_sequence_between_live_ones(gpu, dens):
    """A sequence of 0 frames: its neighbours match the reference, its rows keep the
    sentinel, it adds nothing to the result, on a Chain whose previous compute left
    statistics of a live sequence in its slot."""
    from kfp16 import chain
    b = cr.batch("zero")
    live = cr.batch("mixed")
    ch = chain.Chain(dens.get("den65"), max_seqs=3, max_frames=40)
    check(live, run(gpu, ch, chain.NumBatch(live.fsts[:3]), live, seqs=[0, 1, 2]), seqs=[0, 1, 2])
    out = run(gpu, ch, chain.NumBatch(b.fsts), b)
    check(b, out, family="num:zero")
    assert out[0].frames == 36 and not np.any(out[1][1])


@pytest.mark.parametrize("fit,over", [("fit", "fit+1arc"), ("g1024", "g1025")])
def test_numerator_lds_boundary(gpu, dens, fit, over):
    """The two sides of kf_chain_compute's kernel choice (4S + 3G + 6A + 6 words <= 64 KiB,
    S, G <= 1024): the largest layout that fits and one more arc; G = 1024 and 1025. Both
    match float64; the small companion's gradient rows are bit-identical between the batch
    k_num_fb runs and the one the large FST sends to k_logfb."""
    rows = {}
    for name, lds in ((fit, True), (over, False)):
        b = cr.batch("lds:" + name)
        assert cr.batch_uses_lds(b.fsts) == lds
        _, _, out = compute_batch(gpu, dens, "wide", b)
        check(b, out, family="num:lds")
        r = out[3][0] + np.arange(b.frames[0]) * out[4]
        rows[name] = (out[2][r], out[1][0].copy())
    assert cr.num_lds_words(cr.batch("lds:fit").fsts[1]) == 16384
    np.testing.assert_array_equal(rows[fit][0], rows[over][0])
    np.testing.assert_array_equal(rows[fit][1], rows[over][1])


# ---------------------------------------------------------------- denominator graphs
@pytest.mark.parametrize("leaky", cr.LEAKY)
@pytest.mark.parametrize("case", list(cr.DEN_CASES))
def test_den_graph_families(gpu, dens, case, leaky):
    """Skewed den graphs through the product path with 1, 2 and 3 sequences (a single
    sequence, a ragged pair, a unit with an absent partner) and, for sequence 0, through
    the den ABI with fp32 input."""
    from kfp16 import chain
    b = cr.batch("den:" + case)
    o = dict(leaky=leaky)
    dg = dens.get(case)
    ch = chain.Chain(dg, max_seqs=3, max_frames=16)
    for n in (1, 2, 3):
        nb = chain.NumBatch(b.fsts[:n])
        check(b, run(gpu, ch, nb, b, o, seqs=range(n)), o, seqs=range(n), family="den:" + case)
    g = b.g
    fst = chain.DenFstGPU()
    rc = gpu.core.den_fst_upload(C.byref(fst), g["src"].ctypes.data, g["dst"].ctypes.data,
                                 g["pdf0"].ctypes.data, g["tp"].ctypes.data, g["A"], g["S"], g["P"])
    assert rc == 0, gpu.core.den_last_error()
    x = np.ascontiguousarray(b.xs[0].astype(np.float32))
    post = np.empty_like(x)
    lp = gpu.core.den_forward_backward(C.byref(fst), x.ctypes.data, b.init.ctypes.data, x.shape[0], leaky,
                                       post.ctypes.data)
    gpu.core.den_fst_free(C.byref(fst))
    lp64, post64 = cr.den_f64(g, b.init, x, leaky)
    assert abs(lp - lp64) / x.shape[0] <= 1e-4, (lp, lp64)
    share = np.abs(post - post64) / cr.grad_bar(post64)
    print("den:%s ABI: lp/T %.2e posteriors %.3f of the bar" % (case, abs(lp - lp64) / x.shape[0], share.max()))
    assert share.max() <= 1.0
    np.testing.assert_allclose(post.sum(1), 1.0, atol=1e-4)


def _ring(S, P):
    s = np.arange(S, dtype=np.int32)
    return dict(S=S, P=P, A=S, src=s, dst=((s + 1) % S).astype(np.int32), pdf0=(s % P).astype(np.int32),
                tp=np.full(S, 0.5, np.float32), start=0)


def test_den_graph_limits(gpu):
    """Creation only, no launch of the recursions: the largest graph is accepted, one
    state or pdf more and malformed arcs are rejected with a message."""
    from kfp16 import KfError, chain
    chain.DenGraph(_ring(8191, 4096)).close()
    bad = []
    bad.append(_ring(8192, 64))
    bad.append(_ring(64, 4097))
    for key, val in (("tp", -0.5), ("src", 64), ("src", -1), ("dst", 64), ("pdf0", 64), ("pdf0", -1)):
        g = _ring(64, 64)
        g[key] = g[key].copy()
        g[key][5] = val
        bad.append(g)
    g = _ring(64, 64)
    g["A"] = 0
    bad.append(g)
    for g in bad:
        with pytest.raises(KfError, match="kf_den_graph_create: .+"):
            chain.DenGraph(g)


# ---------------------------------------------------------------- workgroups per unit
def _pick_G(units2, cus):
    """den_pick_G: the most workgroups per unit that keep every workgroup resident."""
    for G in (4, 2):
        if units2 * G <= cus:
            return G
    return 1


@pytest.mark.parametrize("G", [4, 2, 1])
def test_den_workgroups_per_unit(gpu, dens, G):
    """G = 4, 2 and 1 workgroups per unit (sequence pairs, forward and backward co-resident:
    den_pick_G(2 * units)) against float64: first, last and a ragged pair."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nseq = {4: 2, 2: cus // 4 + 16, 1: cus + 44}[G]      # 2, 80, 300 on 256 CUs
    if _pick_G(2 * ((nseq + 1) // 2), cus) != G:
        pytest.skip("%d CUs cannot give G = %d" % (cus, G))
    b = cr.batch("gleg:%d" % nseq)
    ch, _, out = compute_batch(gpu, dens, "den65", b)
    c = ch.debug_census()
    print("G leg %d: %d sequences, census %s" % (G, nseq, c))
    assert c["G"] == G and c["units"] == (nseq + 1) // 2
    sample = cr.g_leg_sample(nseq)
    assert len(sample) == min(6, nseq)
    check(b, out, sample=sample, family="G=%d" % G)
    assert out[0].num_ok == nseq and np.all(out[1][:, 7] == 1.0)


def test_small_graph_xcd_local_exchange(gpu, dens):
    """The den exchange inside one XCD's L2 on a graph whose state rows are too small to
    evict anything from a CU's L1 (65 states): the partial-sum slots, rewritten every other
    frame, must not be served from the reader's L1. G = 4 with every unit's workgroups on
    one XCD (64 sequences on 256 CUs): every sequence against float64, and bit-identical
    to the agent-scope exchange."""
    from kfp16 import chain
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nseq = cus // 4
    b = cr.batch("gleg:%d" % nseq)
    ch = chain.Chain(dens.get("den65"), max_seqs=nseq, max_frames=12)
    nb = chain.NumBatch(b.fsts)
    outs = []
    for force in (False, True):
        ch.debug_exchange_sys(force)
        outs.append(run(gpu, ch, nb, b))
        c = ch.debug_census()
        assert c["G"] == 4 and c["units"] == nseq // 2 and c["forced"] == force
        assert c["local_fwd"] == c["local_bwd"] == c["units"], c   # else nothing ran in the local mode
    ch.debug_exchange_sys(False)
    check(b, outs[0], family="local")
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


# ---------------------------------------------------------------- options and layout
def test_options_and_layout(gpu, dens):
    """Non-default KfChainOpts (folded into k_den_post's epilogue) and leading dimensions /
    row layouts other than ld = ldg = P."""
    from kfp16 import chain
    b = cr.batch("opts")
    ch = chain.Chain(dens.get("den65"), max_seqs=3, max_frames=24)
    nb = chain.NumBatch(b.fsts)
    for name, o in cr.OPTS.items():
        check(b, run(gpu, ch, nb, b, o), o, family="opts:" + name)
    o = cr.OPTS["l2"]
    check(b, run(gpu, ch, nb, b, o, pad=(24, 8)), o, family="opts:padded")
    check(b, run(gpu, ch, nb, b, pad=(24, 8), compact=True), family="opts:compact")
    check(b, run(gpu, ch, nb, b, compact=True), family="opts:compact")


# ---------------------------------------------------------------- batch lifetime
def test_refill_with_other_sizes(gpu, dens):
    """kf_num_batch_refill with smaller, then larger FSTs than the create-time blob: each
    compute is that of the FSTs it was given."""
    from kfp16 import chain
    a = cr.batch("life:a")
    ch = chain.Chain(dens.get("den65"), max_seqs=3, max_frames=12)
    nb = chain.NumBatch(a.fsts)
    check(a, run(gpu, ch, nb, a), family="life")
    for name in ("small", "large", "a"):
        b = cr.batch("life:" + name)
        nb.refill(b.fsts)
        check(b, run(gpu, ch, nb, b), family="life")


def test_new_batch_after_a_freed_one(gpu, dens):
    """A batch freed after a compute and a new one of the same shape (nseq, rows, frames,
    buffers) with other FSTs, as equal-length egs give: the layout cache must not hand the
    new batch the freed one's descriptors (the allocator may return the same address)."""
    from kfp16 import chain
    a, b = cr.batch("life:a"), cr.batch("life:b")
    ch = chain.Chain(dens.get("den65"), max_seqs=3, max_frames=12)
    row0, rows = cr.layout(a.frames, 3)
    x = cr.place(a.xs, row0, 3, rows, a.P)
    assert all(np.array_equal(p, q) for p, q in zip(a.xs, b.xs))      # the same outputs
    dx = gpu.upload_fp16(x)
    og = gpu.upload_fp16(np.full(x.shape, cr.SENTINEL, np.float16))
    outs = []
    for bt in (a, b, a, b):
        nb = chain.NumBatch(bt.fsts)
        ch.compute(nb, dx.ptr, a.P, rows, row0, bt.frames, 3, og.ptr, a.P)
        res = ch.result()
        outs.append((res, ch.seq_stats(3), gpu.read_fp16(og.ptr, x.shape), row0, 3))
        nb.close()                                                      # freed before the next create
        check(bt, outs[-1], family="life")
    assert abs(outs[0][0].objf - outs[1][0].objf) > 1.0                 # A and B do differ
