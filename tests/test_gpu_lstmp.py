"""The projected LSTM sequence operator (include/kf_lstm.h) against a float64 restatement
of its equations with autograd gradients: y, c, dX and every parameter gradient in relative
Frobenius norm under the project's gradient gate of 5e-3 (tests/test_gpu_train_step.py).

Inputs and parameters lie on the fp16 grid, at scales that keep the gates off saturation. Shapes:
one and three 32-cell slices with a K of 96; delay -1 and -3; one step only, 18 step rows across a
16-row tile with T no multiple of |d|, and unequal lengths whose sequences drop out of late steps.
Every case runs twice and must replay bit for bit."""
import numpy as np
import pytest
import torch

from conftest import rel_fro
from kfp16 import lstm

pytestmark = pytest.mark.gpu

D, GATE = 40, 5e-3
SHAPES = [(32, 32, 32), (96, 96, 32)]
LENS = [(3,), (7, 7, 7, 7, 7, 7), (20, 5, 11)]
CASES = [(s, d, l, False) for s in SHAPES for d in (-1, -3) for l in LENS] + [((96, 96, 32), -3, (20, 5, 11), True)]


class _Clip(torch.autograd.Function):
    """identity whose derivative is the row-norm clip; records the norms it saw"""
    @staticmethod
    def forward(ctx, v, th, norms):
        ctx.th, ctx.norms = th, norms
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        n = float(g.norm())
        ctx.norms.append(n)
        return (g * (ctx.th / n) if 0 < ctx.th < n else g), None, None


def reference(p, x, lens, d, dy, clip):
    """float64: (y, c, dx, grads, norms of the recurrent derivative rows before the clip)"""
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    x = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    C, R, norms, ys, cs, row = p["w_ic"].numel(), p["W_r"].shape[0], [], [], [], 0
    for n in lens:
        r, c = [], []
        for t in range(n):
            rp = _Clip.apply(r[t + d], clip, norms) if t + d >= 0 else torch.zeros(R, dtype=torch.float64)
            cp = _Clip.apply(c[t + d], clip, norms) if t + d >= 0 else torch.zeros(C, dtype=torch.float64)
            ai, af, ag, ao = (x[row + t] @ p["W_x"] + rp @ p["W_r"] + p["b"]).split(C)
            i, f, g = torch.sigmoid(ai + p["w_ic"] * cp), torch.sigmoid(af + p["w_fc"] * cp), torch.tanh(ag)
            c.append(f * cp + i * g)
            o = torch.sigmoid(ao + p["w_oc"] * c[t])
            ys.append((o * torch.tanh(c[t])) @ p["W_p"] + p["b_p"])
            r.append(ys[-1][:R])
        cs += c
        row += n
    y = torch.stack(ys)
    (y * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    return (y.detach().numpy(), torch.stack(cs).detach().numpy(), x.grad.numpy(),
            {k: v.grad.numpy() for k, v in p.items()}, norms)


@pytest.mark.parametrize("crn,d,lens,clipped", CASES)
def test_lstmp_forward_backward(gpu, crn, d, lens, clipped):
    kf = gpu
    (C, R, N), T = crn, sum(lens)
    rng = np.random.default_rng(C + 7 * T - d)
    op = lstm.Lstmp(D, C, R, N, d, max_rows=T, max_seqs=len(lens))
    scale = {"W_x": 0.5 / np.sqrt(D), "W_r": 0.5 / np.sqrt(R), "W_p": 1.0 / np.sqrt(C), "b": 0.1, "b_p": 0.1}
    p = {k: (rng.standard_normal(s) * scale.get(k, 0.3)).astype(np.float16).astype(np.float32) for k, s in op.shapes.items()}
    x = rng.standard_normal((T, D)).astype(np.float16)
    dy = rng.standard_normal((T, R + N)).astype(np.float16)
    clip = 0.0
    if clipped:   # below every row norm the unclipped derivative has
        clip = 0.5 * min(reference(p, x, lens, d, dy, 0.0)[4])
        assert clip > 0
    y_ref, c_ref, dx_ref, g_ref, _ = reference(p, x, lens, d, dy, clip)

    op.set_params(p)
    op.set_clip(clip)
    ldx, ldy = D + 8, R + N + 8   # leading dimensions wider than the rows
    xb = kf.upload_fp16(np.pad(x, ((0, 0), (0, 8))))
    dyb = kf.upload_fp16(np.pad(dy, ((0, 0), (0, 8))))
    seq_row0 = np.concatenate([[0], np.cumsum(lens)])
    runs = []
    for _ in range(2):
        yb, dxb = kf.upload_fp16(np.zeros((T, ldy))), kf.upload_fp16(np.zeros((T, ldx)))
        gb = kf.upload_f32(np.zeros(op.num_params))
        op.forward(xb.ptr, ldx, seq_row0, yb.ptr, ldy)
        op.backward(dyb.ptr, ldy, dxb.ptr, ldx, gb.ptr)
        c = op.state()["c"]
        runs.append((kf.read_fp16(yb.ptr, (T, ldy))[:, :R + N], c, kf.read_fp16(dxb.ptr, (T, ldx))[:, :D],
                     kf.read_f32(gb.ptr, (op.num_params,))))
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "a call must replay bit for bit"

    y, c, dx, flat = runs[0]
    errs = {"y": rel_fro(y, y_ref), "c": rel_fro(c, c_ref), "dX": rel_fro(dx, dx_ref)}
    errs.update({"d" + k: rel_fro(v, g_ref[k]) for k, v in op.unflatten(flat).items()})
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= GATE, errs
    op.close()


def test_lstmp_refusals(gpu):
    with pytest.raises(gpu.KfError, match="multiples of 32"):
        lstm.Lstmp(D, 48, 32, 32, -3, 64, 4)
    with pytest.raises(gpu.KfError, match="delay must be negative"):
        lstm.Lstmp(D, 32, 32, 32, 0, 64, 4)
    op = lstm.Lstmp(D, 32, 32, 32, -3, max_rows=8, max_seqs=2)
    op.set_params({k: np.zeros(s, np.float32) for k, s in op.shapes.items()})
    xb, yb = gpu.upload_fp16(np.zeros((9, D))), gpu.upload_fp16(np.zeros((9, 64)))
    with pytest.raises(gpu.KfError, match="max_rows"):
        op.forward(xb.ptr, D, [0, 4, 9], yb.ptr, 64)
    op.close()
