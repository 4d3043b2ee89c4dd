"""tests/attention_ref.py, the reference the per-geometry kernel tests compare with, pinned on
the CPU to things that do not come from the kernels:

  forward   against the oracle (oracle/kf_oracle.c att_forward, itself pinned to the
            reference's loop by test_oracle_attention.py), through a one-layer network whose
            affine is the identity so that proj = x;
  backward  against central finite differences of att_forward's pre-ReLU output in float64,
            at every geometry of the matrix;
  the element bar (|got - r64| <= ulp16(r64) / 2 + 4 E32) against the same mathematics in
            another summation order: the float32 restatement with the key and value columns
            permuted, rounded to fp16, must meet it with 1 E32;
  the mask rule: the elements it leaves out (|y64| <= 4 E32) are at most 0.1 % of a case."""
import numpy as np
import pytest

import attention_ref as AR
import oracle
from attention_ref import CASES, CASE_IDS


def _xcfg(case):
    H, kd, vd, T, nl, nr, st = case
    ctx, A, od, width = AR.dims(H, kd, vd, nl, nr)
    return (f"input name=input dim={H * A}\n"
            f"attention-relu-batchnorm-layer name=att num-heads={H} value-dim={vd} key-dim={kd} "
            f"num-left-inputs={nl} num-right-inputs={nr} time-stride={st}\n"
            "output-layer name=output dim=8 include-log-softmax=false\n")


@pytest.mark.parametrize("i", [2, 7, 9], ids=lambda i: CASE_IDS[i])
def test_forward_matches_oracle(i):
    """g3 (dead positions in every frame), g8 (T far below the context) and g10 (no value part)"""
    case = CASES[i]
    H, kd, vd, T, nl, nr, st = case
    ctx, A, od, width = AR.dims(H, kd, vd, nl, nr)
    inp, _ = AR.case_reference(i)
    rng = np.random.default_rng(i)
    mean, var = rng.uniform(-0.2, 0.2, width).astype(np.float32), rng.uniform(0.5, 2.0, width).astype(np.float32)
    gamma, beta = inp["scale"], inp["shift"]      # a quarter of the gammas negative
    params = {"att.W": np.eye(H * A, dtype=np.float32), "att.Bias": np.zeros((1, H * A), np.float32),
              "output.W": np.zeros((width, 8), np.float32), "output.Bias": np.zeros((1, 8), np.float32)}
    on = oracle.OracleNet(_xcfg(case), params, {("att", 0): (mean, var, gamma, beta)}, round_mode=oracle.ROUND_NONE)
    on.forward(inp["proj"].astype(np.float32))
    scale = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-3)
    shift = beta - mean * scale
    y, out, bits = AR.att_forward(inp["proj"], H, kd, vd, nl, nr, st, inp["s"], scale, shift, np.float64)
    np.testing.assert_allclose(on.act("att"), out, rtol=2e-5, atol=2e-6)
    m = on.mask("att")
    if m is not None:   # the oracle's ReLU decisions, where the pre-activation is clear of zero
        clear = np.abs(y) > 1e-5
        assert np.array_equal(m.reshape(T, width).astype(bool)[clear], (y > 0)[clear])
    assert np.array_equal(np.unpackbits(bits, axis=1, bitorder="little")[:, :width].astype(bool), y > 0)
    on.close()


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_backward_matches_finite_differences(i):
    """loss = sum dz * y (pre-ReLU), central differences with step 1e-4 in float64: their error is
    O(step^2) = 1e-8 of the third derivative, two orders below the bar 1e-6 max |grad|. The 12
    largest-magnitude gradient coordinates and 12 random ones."""
    case = CASES[i]
    H, kd, vd, T, nl, nr, st = case
    inp, ref = AR.case_reference(i)
    g = ref["g64"]
    proj, dz = inp["proj"].astype(np.float64), inp["dz"].astype(np.float64)

    def loss(p):
        y, _, _ = AR.att_forward(p, H, kd, vd, nl, nr, st, inp["s"], inp["scale"], inp["shift"], np.float64)
        return float(np.sum(dz * y))

    rng = np.random.default_rng(2)
    picks = [np.unravel_index(k, g.shape) for k in np.argsort(-np.abs(g).ravel())[:12]]
    picks += [(int(rng.integers(g.shape[0])), int(rng.integers(g.shape[1]))) for _ in range(12)]
    bar, step = 1e-6 * np.abs(g).max(), 1e-4
    for t, c in picks:
        pp, pm = proj.copy(), proj.copy()
        pp[t, c] += step
        pm[t, c] -= step
        num = (loss(pp) - loss(pm)) / (2 * step)
        assert abs(num - g[t, c]) <= bar, ((int(t), int(c)), num, g[t, c], bar)


def test_context_one_gradient_is_exactly_zero():
    """ctx 1: w == 1, so db = w (dw - w dw) = 0 and d key, d query key and d query context are
    exactly zero in every dtype; only d value = dz_v is not."""
    case = CASES[0]
    assert 1 + case[4] + case[5] == 1
    _, ref = AR.case_reference(0)
    parts = AR.bwd_parts(case)
    for k in ("64", "32"):
        for name in ("key", "query key", "query context"):
            assert not ref["g" + k][:, parts[name]].any(), (k, name)
        assert ref["g" + k][:, parts["value"]].any()


def _permuted_f32(case, inp, seed):
    """The float32 restatement with the key (and query key) columns and the value columns (with
    dz_v and the output's value columns) permuted, un-permuted again: the same mathematics, the
    dot products summed in another order. Returns (y, out, g), unrounded."""
    H, kd, vd, T, nl, nr, st = case
    ctx, A, od, width = AR.dims(H, kd, vd, nl, nr)
    rng = np.random.default_rng(seed)
    pk, pv = rng.permutation(kd), rng.permutation(vd)
    ca = np.arange(A)           # column permutation of a head's affine row
    ca[:kd], ca[kd:kd + vd], ca[kd + vd:2 * kd + vd] = pk, kd + pv, kd + vd + pk
    co = np.arange(od)
    co[:vd] = pv
    ca = (np.arange(H)[:, None] * A + ca[None, :]).ravel()
    co = (np.arange(H)[:, None] * od + co[None, :]).ravel()
    y, out, _ = AR.att_forward(inp["proj"][:, ca], H, kd, vd, nl, nr, st, inp["s"], inp["scale"][co],
                               inp["shift"][co], np.float32)
    g = AR.att_backward(inp["proj"][:, ca], inp["dz"][:, co], H, kd, vd, nl, nr, st, inp["s"], np.float32)
    iy, io, ig = np.empty_like(y), np.empty_like(out), np.empty_like(g)
    iy[:, co], io[:, co], ig[:, ca] = y, out, g
    return iy.astype(np.float64), io.astype(np.float64), ig.astype(np.float64)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_element_bar_holds_for_another_summation_order(i):
    """The bar's self-check: fp16(permuted float32 restatement) is within ulp16 / 2 + 1 E32 of the
    float64 reference in every part, forward and backward (the kernels get 4 E32). If this
    failed, the bar or the reference would be wrong, not a kernel."""
    case = CASES[i]
    inp, ref = AR.case_reference(i)
    y, out, g = _permuted_f32(case, inp, 50 + i)
    r16 = lambda a: a.astype(np.float16).astype(np.float64)
    worst = {}
    for name, sel in AR.fwd_parts(case).items():
        worst[name] = AR.element_excess(r16(out)[:, sel], ref["out64"][:, sel], ref["out32"][:, sel])
    for name, sel in AR.bwd_parts(case).items():
        worst[name] = AR.element_excess(r16(g)[:, sel], ref["g64"][:, sel], ref["g32"][:, sel])
    print(CASE_IDS[i], {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_mask_rule_excludes_little(i):
    """The kernel tests compare ReLU bits only where |y64| > 4 E32; on the reference inputs that
    leaves out at most 0.1 % of a case, and there float64 and float32 agree on every bit."""
    case = CASES[i]
    _, ref = AR.case_reference(i)
    inc = AR.mask_included(case, ref["y64"], ref["y32"])
    assert (~inc).mean() <= AR.MASK_EXCLUDED_MAX, (~inc).sum()
    assert np.array_equal((ref["y64"] > 0)[inc], (ref["y32"] > 0)[inc])


def test_ulp16():
    x = np.array([0.0, 2.0 ** -30, 2.0 ** -14, 0.75, 1.0, 1.5, -2.0, 1000.0, 65504.0])
    want = np.array([2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.5, 32.0])
    assert np.array_equal(AR.ulp16(x), want)
    near = np.float16([0.75, 1.0, 1.5, 1000.0])   # numpy's own fp16 spacing
    assert np.array_equal(AR.ulp16(near), np.spacing(near).astype(np.float64))
