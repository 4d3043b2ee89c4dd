"""kf_chain_set_grad_scale (kf_chain.h): the loss scale inside the objective's
kernels (k_den_post's gradient assembly, k_chain_xent), on the cases of tests/chain_ref.py:
chain20, lattice40, the ragged T = 1, 2, 7, 8, 9 set, the first two sequences of the skewed den
graph s65 (a sequence pair), and the P = 200 batch of test_gpu_chain_weights.py (k_chain_xent's
vector path; the other cases' P = 129 / 33 take its scalar path).

A pointer to 1.0: every output bit-identical to no pointer. A pointer to 2^6: statistics, result
and xent objective bit-identical to off; every gradient element within
2^6 * (w * 1e-4) + one fp16 ulp of the scaled value of 2^6 x the float64 derivative, which is
the existing bar (chain_ref.grad_bar; for the xent gradient with w * xent_regularize, as
test_gpu_chain_xent.py) times the scale. The same through the weighted call with non-trivial
frame and sequence weights, and on the compact-row layout."""
import numpy as np
import pytest
import torch  # noqa: F401  (the HIP runtime first: the libraries then bind the same copy)

import chain_ref as cr
import xent_ref as xr_

pytestmark = pytest.mark.gpu

XR = 0.1
SCALE = 64.0


class _Case:
    def __init__(self, name):
        if name == "p200":
            from kfp16 import synth
            self.g = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=200)
            self.init = cr.den_init(self.g)
            self.fsts = [xr_._lattice(301, 200, 9), cr.weighted_chain(302, 4, 200), cr.weighted_chain(303, 2, 200)]
            self.frames = np.array([9, 4, 1], np.int32)
            self.xs = [cr.outputs(310 + i, int(T), 200) for i, T in enumerate(self.frames)]
            self.l2 = 5e-4
        else:
            bname, _, nseq = name.partition("/")
            b = cr.batch(bname)
            idx = list(range(int(nseq))) if nseq else list(range(len(b.fsts)))
            self.g, self.init = b.g, b.init
            self.fsts = [b.fsts[i] for i in idx]
            self.frames = b.frames[idx]
            self.xs = [b.xs[i] for i in idx]
            self.l2 = 0.0
        self.P = int(self.g["P"])
        self.ys = [xr_.xent_outputs(900 + i, int(T), self.P) for i, T in enumerate(self.frames)]
        self._ref = {}

    def ref(self, i, w):
        """(-deriv of the chain objective, xent gradient) of sequence i at weight w, float64"""
        if (i, w) not in self._ref:
            d64, _ = cr.objf_f64(self.g, self.init, self.fsts[i], self.xs[i], self.l2, 0.01, 1e-5, w)
            xg, _, _ = xr_.xent_f64(self.fsts[i], self.xs[i], self.ys[i], XR, w)
            self._ref[(i, w)] = (-d64, xg)
        return self._ref[(i, w)]


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


class _Run:
    def __init__(self, gpu, c, compact=False):
        from kfp16 import chain as kc
        self.gpu, self.c = gpu, c
        self.stride = 1 if compact else 3
        self.row0, self.rows = cr.layout(c.frames, self.stride, compact=compact)
        self.dg = kc.DenGraph(c.g, c.init)
        self.ch = kc.Chain(self.dg, max_seqs=len(c.fsts), max_frames=int(c.frames.max()))
        self.nb = kc.NumBatch(c.fsts)
        self.dx = gpu.upload_fp16(cr.place(c.xs, self.row0, self.stride, self.rows, c.P))
        self.dy = gpu.upload_fp16(cr.place(c.ys, self.row0, self.stride, self.rows, c.P, seed=1))
        self.opts = kc.KfChainOpts(c.l2, 0.01, 1e-5, XR, 1.0)

    def seq_rows(self, i):
        return self.row0[i] + np.arange(self.c.frames[i]) * self.stride

    def run(self, scale=None, **weights):
        """scale None: kf_chain_set_grad_scale(NULL); else a device float holding it"""
        gpu, c, P = self.gpu, self.c, self.c.P
        sbuf = None if scale is None else gpu.upload_f32(np.array([scale], np.float32))
        self.ch.set_grad_scale(None if sbuf is None else sbuf.ptr)
        og = gpu.upload_fp16(np.full((self.rows, P), cr.SENTINEL, np.float16))
        xg = gpu.upload_fp16(np.full((self.rows, P), cr.SENTINEL, np.float16))
        self.ch.compute(self.nb, self.dx.ptr, P, self.rows, self.row0, c.frames, self.stride, og.ptr, P, self.opts,
                        **weights)
        out = dict(res=self.ch.result(), stats=self.ch.seq_stats(len(c.fsts)).copy())
        self.ch.xent(self.nb, self.dy.ptr, P, xg.ptr, P, self.opts)
        out["xres"] = self.ch.xent_result()
        out["grad"], out["xgrad"] = gpu.read_fp16(og.ptr, (self.rows, P)), gpu.read_fp16(xg.ptr, (self.rows, P))
        self.ch.set_grad_scale(None)   # (sbuf is freed when this returns)
        return out

    def close(self):
        for h in (self.ch, self.nb, self.dg):
            h.close()


def _res_tuple(r):
    return (r.objf, r.l2_term, r.total_weight, r.num_logprob, r.den_logprob, r.frames, r.out_of_range,
            r.num_ok, r.num_seqs)


def _same_stats(a, b):
    np.testing.assert_array_equal(a["stats"].view(np.uint32), b["stats"].view(np.uint32))
    assert _res_tuple(a["res"]) == _res_tuple(b["res"])
    assert a["xres"] == b["xres"]


def _check(r, seq_w=None, frame_w=None, what=""):
    """the two checks of the module docstring on one layout and one set of weights"""
    c = r.c
    kw = {}
    if seq_w is not None or frame_w is not None:
        kw = dict(seq_weight=seq_w, frame_weight=None if frame_w is None else np.concatenate(frame_w))
    off = r.run(None, **kw)
    assert off["res"].num_ok == len(c.fsts)
    one = r.run(1.0, **kw)
    for k in ("grad", "xgrad"):
        np.testing.assert_array_equal(one[k].view(np.uint16), off[k].view(np.uint16), err_msg=f"{what}: {k} at 1.0")
    _same_stats(one, off)
    got = r.run(SCALE, **kw)
    _same_stats(got, off)
    sup = np.zeros(r.rows, bool)
    for i, T in enumerate(c.frames):
        w = 1.0 if seq_w is None else float(seq_w[i])
        f = np.ones((int(T), 1)) if frame_w is None else frame_w[i].astype(np.float64)[:, None]
        rows = r.seq_rows(i)
        sup[rows] = True
        gref, xref = c.ref(i, w)
        for k, ref, wbar in (("grad", gref, w), ("xgrad", xref, w * XR)):
            want = SCALE * ref * f
            d = np.abs(got[k][rows].astype(np.float64) - want)
            share = d / cr.grad_bar(want, SCALE * wbar)
            print(f"{what} seq {i} {k}: max |d| {d.max():.2e}, {share.max():.3f} of the bar")
            assert share.max() <= 1.0, (what, i, k, float(share.max()))
            assert np.all(np.isfinite(got[k][rows]))
            assert np.any(got[k][rows] != off[k][rows])
    for k in ("grad", "xgrad"):
        assert np.all(got[k][~sup] == cr.SENTINEL), k
    return off, got


@pytest.mark.parametrize("name", ["chain20", "lattice40", "ragged", "den:s65/2", "p200"])
def test_scale_one_is_off_and_scale_64_scales(gpu, name):
    r = _Run(gpu, _case(name))
    off, got = _check(r, what=name)
    # a power of two commutes with the rounding outside fp16's subnormal range and below its
    # overflow: there the scaled element is exactly the unscaled one times 2^6
    for k in ("grad", "xgrad"):
        a, b = off[k].astype(np.float32), got[k].astype(np.float32)
        exact = (np.abs(a) >= 2.0 ** -14) & (np.abs(a) * SCALE < 65504) & (a != cr.SENTINEL)
        assert exact.any()
        np.testing.assert_array_equal(b[exact], a[exact] * np.float32(SCALE), err_msg=k)
    r.close()


@pytest.mark.parametrize("name", ["ragged", "p200"])
def test_weighted_call(gpu, name):
    """kf_chain_compute_weighted: a ramp of frame weights and sequence weights that are no powers of two"""
    c = _case(name)
    seq_w = np.array([1.0, 0.5, 2.0, 0.75, 1.5], np.float32)[:len(c.fsts)]
    frame_w = [np.linspace(0.1, 1.0, int(T)).astype(np.float32) for T in c.frames]
    r = _Run(gpu, c)
    _check(r, seq_w, frame_w, what=name + " weighted")
    r.close()


@pytest.mark.parametrize("name", ["ragged", "p200"])
def test_compact_row_layout(gpu, name):
    r = _Run(gpu, _case(name), compact=True)
    assert r.stride == 1 and r.rows == int(_case(name).frames.sum())
    _check(r, what=name + " compact")
    r.close()

