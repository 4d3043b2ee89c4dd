"""kf_chain_xent (k_chain_xent, csrc/chain_xent.hip) against the float64 reference
of tests/xent_ref.py, after a real kf_chain_compute on the cases of xent_ref.CASES: weighted
chains and lattices (labels 0 and P + 3: out-of-range groups), a sequence the objective marks
bad, a zero-frame sequence, P = 8, 13 (the scalar path), 200, 3080 and 4096 (two column chunks
of the LDS row), 1, 2 and 9 frames, a stride-3 layout with lead rows and the compact layout,
ldx and ldg above P, xr = 0.1 and 0, w = 1 and 0.5. (P = 4104 cannot be run: a den graph, and
so a KfChain, takes at most 4096 pdfs; 4096 stands in for it.)

Bars: every gradient element within chain_ref.grad_bar(ref, w * xr) = w * xr * 1e-4
plus one fp16 ulp of the value; the xent objective within 1e-3 per frame; the weight exact;
rows without supervision and pad columns keep their sentinel; a second call is bit-identical.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (the HIP runtime first: the libraries then bind the same copy)

import chain_ref as cr
import xent_ref as xr_

pytestmark = pytest.mark.gpu


def _run(gpu, c):
    """compute + xent (twice) of case c. Returns (gradient buffers of both calls, results of
    both calls, per-sequence chain statistics, row0, stride)."""
    from kfp16 import chain
    stride = 1 if c.compact else 3
    row0, rows = cr.layout(c.frames, stride, compact=c.compact)
    P, ldx, ldg = c.P, c.P + c.pad[0], c.P + c.pad[1]
    dg = chain.DenGraph(c.g, c.init)
    ch = chain.Chain(dg, max_seqs=len(c.fsts), max_frames=int(max(c.frames.max(), 1)))
    nb = chain.NumBatch(c.fsts)
    dx = gpu.upload_fp16(cr.place(c.xs, row0, stride, rows, P))
    dy = gpu.upload_fp16(cr.place(c.ys, row0, stride, rows, P, ldx, seed=1))
    og = gpu.upload_fp16(np.full((rows, P), cr.SENTINEL, np.float16))
    opts = chain.KfChainOpts(0.0, 0.01, 1e-5, c.xr, c.w)
    ch.compute(nb, dx.ptr, P, rows, row0, c.frames, stride, og.ptr, P, opts)
    grads, results = [], []
    for _ in range(2):
        xg = gpu.upload_fp16(np.full((rows, ldg), cr.SENTINEL, np.float16))
        ch.xent(nb, dy.ptr, ldx, xg.ptr, ldg, opts)
        results.append(ch.xent_result())
        grads.append(gpu.read_fp16(xg.ptr, (rows, ldg)))
    stats = ch.seq_stats(len(c.fsts)).astype(np.float64)
    ch.close()
    nb.close()
    dg.close()
    return grads, results, stats, row0, stride


@pytest.mark.parametrize("name", list(xr_.CASES))
def test_xent_against_float64(gpu, name):
    c = xr_.case(name)
    grads, results, stats, row0, stride = _run(gpu, c)
    got, P = grads[0], c.P
    sup = np.zeros(got.shape[0], bool)
    objf = weight = 0.0
    worst = wabs = 0.0
    for i, T in enumerate(c.frames):
        rows = row0[i] + np.arange(T) * stride
        sup[rows] = True
        if T == 0:
            continue
        ref, o, _ = c.ref(i)
        assert stats[i, 7] == (0.0 if i == c.bad else 1.0), (i, stats[i])
        objf += o
        weight += float(np.float32(c.w)) * T
        d = np.abs(got[rows, :P].astype(np.float64) - ref)
        bar = cr.grad_bar(ref, c.w * c.xr)
        if i == c.bad or c.xr == 0:
            assert not np.any(got[rows, :P]), i          # written, as zeros
        else:
            assert np.any(got[rows, :P]), i
            worst, wabs = max(worst, float((d / bar).max())), max(wabs, float(d.max()))
        assert np.all(d <= bar), (i, float(d.max()), np.unravel_index((d - bar).argmax(), d.shape))
    frames = int(c.frames.sum())
    print("%s: gradient %.3f of its bar (|d| %.2e), objective/frame |d| %.2e" % (
        name, worst, wabs, abs(results[0][0] - objf) / frames))
    assert abs(results[0][0] - objf) / frames <= 1e-3, (results[0][0], objf)
    assert objf < 0.0 and results[0][1] == weight
    assert np.all(got[~sup] == cr.SENTINEL)              # rows without supervision
    assert np.all(got[:, P:] == cr.SENTINEL)             # pad columns
    np.testing.assert_array_equal(grads[0].view(np.uint16), grads[1].view(np.uint16))
    assert results[0] == results[1]


def test_xent_refusals(gpu):
    """No compute before the call, another batch than the compute's, leading dimensions below
    P, null pointers: -1 with the cause in the text; nothing is written."""
    from kfp16 import KfError, chain
    c = xr_.case("p13_stride3")
    row0, rows = cr.layout(c.frames, 3)
    dg = chain.DenGraph(c.g, c.init)
    ch = chain.Chain(dg, max_seqs=len(c.fsts), max_frames=int(c.frames.max()))
    nb, other = chain.NumBatch(c.fsts), chain.NumBatch(c.fsts)
    P = c.P
    dx = gpu.upload_fp16(cr.place(c.xs, row0, 3, rows, P))
    dy = gpu.upload_fp16(cr.place(c.ys, row0, 3, rows, P))
    og = gpu.upload_fp16(np.full((rows, P), cr.SENTINEL, np.float16))
    xg = gpu.upload_fp16(np.full((rows, P), cr.SENTINEL, np.float16))
    opts = chain.KfChainOpts(0.0, 0.01, 1e-5, 0.1, 1.0)
    with pytest.raises(KfError, match="no kf_chain_compute before"):
        ch.xent(nb, dy.ptr, P, xg.ptr, P, opts)
    ch.compute(nb, dx.ptr, P, rows, row0, c.frames, 3, og.ptr, P, opts)
    with pytest.raises(KfError, match="no kf_chain_xent since"):
        ch.xent_result()
    with pytest.raises(KfError, match="not the one of the last kf_chain_compute"):
        ch.xent(other, dy.ptr, P, xg.ptr, P, opts)
    with pytest.raises(KfError, match="below P"):
        ch.xent(nb, dy.ptr, P - 1, xg.ptr, P, opts)
    with pytest.raises(KfError, match="below P"):
        ch.xent(nb, dy.ptr, P, xg.ptr, P - 1, opts)
    with pytest.raises(KfError, match="NULL argument"):
        ch.xent(nb, None, P, xg.ptr, P, opts)
    with pytest.raises(KfError, match="NULL argument"):
        ch.xent(nb, dy.ptr, P, None, P, opts)
    assert np.all(gpu.read_fp16(xg.ptr, (rows, P)) == cr.SENTINEL)
    ch.xent(nb, dy.ptr, P, xg.ptr, P, opts)              # and the call they refused still works
    assert ch.xent_result()[1] == float(c.frames.sum())
    for h in (ch, nb, other, dg):
        h.close()
