"""The float64 restatement of the conv components' natural gradient, on its own (no GPU)."""
import numpy as np
import pytest

import natgrad_conv_ref as C
import natgrad_ref as R


@pytest.mark.parametrize("Din, N", [(10, 16), (55, 48), (54, 48), (300, 64)])
def test_two_sided_step(Din, N):
    rng = np.random.default_rng(Din)
    basis = np.linalg.qr(rng.standard_normal((N, 6)))[0].T
    ref = C.ConvPre(Din, N)
    assert (ref.pin is None) == (Din // 2 < 8) and ref.pout.R == min(80, N // 2)
    for step in range(7):
        G = R.low_rank_batch(rng, Din, N, basis)
        before = [None if p is None else p.copy() for p in (ref.pin, ref.pout)]
        Gh, info = ref.step(G)
        Pin, Pout = (None if p is None else p.proj() for p in before)
        gin, gout = (info[s]["gamma"] if s in info else 1.0 for s in ("in", "out"))
        want = R.precondition_gradient(G, gin, gout, Pin, Pout)
        assert np.linalg.norm(Gh - want) <= 1e-12 * np.linalg.norm(want)
        # the out side saw G1 without gamma_in, and N counts the rows of each side's X
        G1 = G if Pin is None else G - Pin @ G
        assert abs(info["out"]["trx"] - np.sum(G1 * G1)) <= 1e-12 * np.sum(G1 * G1) and info["out"]["N"] == Din
        assert np.allclose(info["out"]["L"], before[1].W @ G1.T @ G1 @ before[1].W.T, rtol=1e-10, atol=0)
        if ref.pin is not None:
            assert info["in"]["N"] == N and abs(info["in"]["trx"] - np.sum(G * G)) <= 1e-12 * np.sum(G * G)
        for p, rows in ((ref.pin, N), (ref.pout, Din)):
            if p is not None:
                assert p.t == step + 1 and abs(p.eta(rows) - (1.0 - np.exp(-0.25))) < 1e-15
    assert gout > 1.0 and (ref.pin is None or gin > 1.0)
