"""The global-rows denominator (kf_den_graph_create_rows, chain_den_global.hip)
through kf_chain_compute, against the float64 references of tests/chain_ref.py with the bars of
tests/test_gpu_chain_graphs.py (its header; run / check are imported from there): den log-prob
1e-4 per frame, objective 1e-3 per frame, every gradient element within chain_ref.grad_bar,
sentinel rows and pad columns untouched, the statistics exact where they are exact there.

A gradient scaled by a factor k (a frame weight, the grad scale) is rne_fp16(-(d k)) of the fp32
derivative d, so its bar is the unscaled one times k: grad_bar(k ref, k w).
"""
import numpy as np
import pytest
import torch  # noqa: F401  (the HIP runtime first: the libraries then bind the same copy)

import chain_ref as cr
from test_gpu_chain_graphs import check, run

pytestmark = pytest.mark.gpu

P65 = cr.DEN65["P"]
BIG = {"P4097": (64, 4097), "S8192": (8192, 64), "both": (8200, 4100)}   # beyond the LDS path
_big = {}


def _big_batch(name):
    """cr.skewed_den at (S, P), A = 3 S + 8, its pdfs spread over all of [0, P) (skewed_den uses
    the first `used`; A bounds it), 3 ragged sequences."""
    if name not in _big:
        S, P = BIG[name]
        A = 3 * S + 8
        g = cr.skewed_den(900 + S % 7, S, P, A=A, used=min(P, A - 6))
        g["pdf0"] = np.random.default_rng(S).permutation(P)[g["pdf0"]].astype(np.int32)
        _big[name] = cr.Batch("big:" + name, g, [(cr.weighted_chain(90 + i, 3, P), T, 950 + i)
                                                  for i, T in enumerate((5, 8, 3))])
    return _big[name]


def _chain(b, rows, max_seqs=None, max_frames=None):
    from kfp16 import chain
    dg = chain.DenGraph(b.g, b.init, rows=rows)
    return dg, chain.Chain(dg, max_seqs=max_seqs or len(b.fsts), max_frames=max_frames or int(max(b.frames.max(), 1)))


@pytest.mark.parametrize("rows", ["global", "auto"])
@pytest.mark.parametrize("name", list(BIG))
def test_beyond_the_lds_limits(gpu, name, rows):
    from kfp16 import chain
    b = _big_batch(name)
    dg, ch = _chain(b, rows)
    assert dg.rows == "global"
    check(b, run(gpu, ch, chain.NumBatch(b.fsts), b))
    c = ch.debug_census()
    assert c["units"] == c["G"] == c["local_fwd"] == c["local_bwd"] == 0


@pytest.mark.parametrize("leaky", cr.LEAKY)
@pytest.mark.parametrize("case", list(cr.DEN_CASES))
def test_forced_global_on_the_den_families(gpu, case, leaky):
    """Skew, dead ends, unused pdfs, all-zero row groups; 1, 2 and 3 sequences (NQ = 1, 2, 4)."""
    from kfp16 import chain
    b = cr.batch("den:" + case)
    o = dict(leaky=leaky)
    if leaky == cr.LEAKY[0]:
        auto = chain.DenGraph(b.g, b.init, rows="auto")
        assert auto.rows == "lds"
        auto.close()
    dg, ch = _chain(b, "global")
    assert dg.rows == "global"
    for n in (1, 2, 3):
        check(b, run(gpu, ch, chain.NumBatch(b.fsts[:n]), b, o, seqs=range(n)), o, seqs=range(n))


@pytest.mark.parametrize("nseq", [1, 2, 3, 63, 64, 65])
def test_sequence_group_edges(gpu, nseq):
    """NQ = 1, 2, 4, 64 and a second group with one sequence; sequence 1 is shorter."""
    from kfp16 import chain
    b = cr.Batch("dg:%d" % nseq, cr.den_graph("den65"),
                 [(cr.weighted_chain(100 + i, 4, P65), 4 if i == 1 else 6, 1000 + i) for i in range(nseq)])
    _, ch = _chain(b, "global")
    out = run(gpu, ch, chain.NumBatch(b.fsts), b)
    check(b, out, sample=sorted({0, nseq // 2, nseq - 1}))
    assert out[0].num_ok == nseq


def _asm_batch(frames=(8, 5, 7)):
    return cr.Batch("dg:asm%s" % (frames,), cr.den_graph("den65"),
                    [(cr.weighted_chain(61 + i, 4, P65), T, 260 + i) for i, T in enumerate(frames)])


@pytest.mark.parametrize("name,o,kw", [
    ("l2", cr.OPTS["l2"], {}), ("oor+weight", cr.OPTS["w2"], {}), ("compact", {}, dict(compact=True)),
    ("padded", cr.OPTS["l2"], dict(pad=(24, 8))), ("padded-compact", {}, dict(pad=(24, 8), compact=True))])
def test_assembly_options_and_layouts(gpu, name, o, kw):
    from kfp16 import chain
    b = _asm_batch()
    _, ch = _chain(b, "global")
    check(b, run(gpu, ch, chain.NumBatch(b.fsts), b, o, **kw), o)


def test_zero_frame_sequence_between_live_ones(gpu):
    from kfp16 import chain
    live, b = _asm_batch(), _asm_batch((8, 0, 7))
    _, ch = _chain(live, "global")
    check(live, run(gpu, ch, chain.NumBatch(live.fsts), live))     # leaves statistics in slot 1
    out = run(gpu, ch, chain.NumBatch(b.fsts), b)
    check(b, out)
    assert out[0].frames == 15 and not np.any(out[1][1])


@pytest.mark.parametrize("what", ["seq_weight", "frame_weight", "grad_scale", "not_finite"])
def test_weights_scale_and_not_finite(gpu, what):
    """kf_chain_compute_weighted, kf_chain_set_grad_scale and the all-zero rows of a not-finite
    sequence: sequence i against the float64 reference at weight w_i, its rows times the frame
    weight or the scale."""
    from kfp16 import chain
    b = _asm_batch()
    o = cr.OPTS["l2"]
    sw = np.array([0.5, 2.0, 1.25], np.float32) if what == "seq_weight" else np.ones(3, np.float32)
    fw = np.ones(int(b.frames.sum()), np.float32)
    if what == "frame_weight":
        fw = np.random.default_rng(5).choice(np.array([0.0, 0.5, 1.0, 1.75], np.float32), len(fw))
        fw[:2] = (0.0, 0.5)
    k = 4.0 if what == "grad_scale" else 1.0
    xs = [x.copy() for x in b.xs]
    if what == "not_finite":
        xs[1][0, b.fsts[1]["pdf1"][0] - 1] = np.inf   # on the numerator path of sequence 1
    _, ch = _chain(b, "global")
    nb = chain.NumBatch(b.fsts)
    row0, rows = cr.layout(b.frames, 3)
    dx = gpu.upload_fp16(cr.place(xs, row0, 3, rows, P65))
    og = gpu.upload_fp16(np.full((rows, P65), cr.SENTINEL, np.float16))
    sbuf = gpu.upload_f32(np.array([k], np.float32))
    ch.set_grad_scale(sbuf.ptr if what == "grad_scale" else None)
    ch.compute(nb, dx.ptr, P65, rows, row0, b.frames, 3, og.ptr, P65, chain.KfChainOpts(o["l2"], o["oor"], o["leaky"], 0.0, o["weight"]),
               seq_weight=sw if what == "seq_weight" else None, frame_weight=fw if what == "frame_weight" else None)
    res, stats, got = ch.result(), ch.seq_stats(3).astype(np.float64), gpu.read_fp16(og.ptr, (rows, P65))
    ch.set_grad_scale(None)
    sup = np.zeros(rows, bool)
    for i, T in enumerate(b.frames):
        r = row0[i] + np.arange(T) * 3
        sup[r] = True
        w = float(np.float32(o["weight"]) * sw[i])
        s = stats[i]
        if what == "not_finite" and i == 1:
            assert not np.any(got[r]) and s[7] == 0.0 and s[2] == -10.0 * w * T and s[3] == 0.0
            continue
        d64, ref = b.ref(i, **dict(o, weight=w))
        assert abs(s[1] - ref["den_logprob"]) / T <= 1e-4 and abs(s[2] - ref["objf"]) / T <= 1e-3, (i, s, ref)
        assert s[7] == 1.0 and s[4] == float(np.float32(w)) * T and abs(s[3] - ref["l2_term"]) <= 1e-3 * abs(ref["l2_term"])
        f = (fw[b.frames[:i].sum():][:T] * k)[:, None].astype(np.float64)
        err, bar = np.abs(got[r].astype(np.float64) + d64 * f), cr.grad_bar(d64 * f, w * f)
        print("%s seq %d: largest gradient error %.2e, smallest margin %.2e" % (what, i, err.max(), (bar - err).min()))
        assert np.all(err <= bar), (i, np.unravel_index((err - bar).argmax(), err.shape))
    assert np.all(got[~sup] == cr.SENTINEL)
    assert res.num_ok == (2 if what == "not_finite" else 3)


def test_replay_is_bit_identical(gpu):
    """The same compute twice, and once more after a batch of another shape (the layout cache)."""
    from kfp16 import chain
    b = _big_batch("both")
    _, ch = _chain(b, "global")
    nb = chain.NumBatch(b.fsts)
    o = cr.OPTS["l2"]
    outs = [run(gpu, ch, nb, b, o), run(gpu, ch, nb, b, o)]
    run(gpu, ch, chain.NumBatch(b.fsts[:2]), b, o, seqs=[1, 0], compact=True)
    outs.append(run(gpu, ch, nb, b, o))
    for out in outs[1:]:
        np.testing.assert_array_equal(out[1], outs[0][1])
        np.testing.assert_array_equal(out[2], outs[0][2])
