"""The dynamic loss scale's rule without a device: tests/loss_scale_ref.py against
the exported host scaler kaldi_loss_scaler_update (the reference's LossScaler, whose rule
tests/test_abi.py pins), and TrainConfig's validation of the new fields."""
import numpy as np
import pytest

from loss_scale_ref import LossScaleRef, overflow_of


def _host_run(init, pattern):
    from kfp16 import bridge_abi as kb
    ls = kb.cgo.kaldi_loss_scaler_create(float(init))
    out = []
    for ov in pattern:
        kb.cgo.kaldi_loss_scaler_update(ls, int(ov))
        out.append(kb.cgo.kaldi_loss_scaler_get_scale(ls))
    kb.cgo.kaldi_loss_scaler_free(ls)
    return out


def _ref_run(pattern, **opts):
    r = LossScaleRef(**opts)
    out = []
    for ov in pattern:
        r.update(ov)
        out.append(float(r.scale))
    return out, r


def test_scripted_sequence_against_host_scaler():
    """from 4: two overflows to the floor 1 and one more held there, 2000 clean steps double it, an
    overflow at clean step 1999 resets the count; from 32768: growth to the ceiling and held"""
    pat = [1, 1, 1] + [0] * 2000 + [0] * 1999 + [1] + [0] * 1999 + [0]
    got, r = _ref_run(pat, init_scale=4.0)
    assert got == _host_run(4.0, pat)
    assert got[2] == 1.0 and got[1] == 1.0 and got[0] == 2.0        # the lower clamp, reached and held
    assert got[3 + 1999] == 2.0 and got[3 + 1998] == 1.0            # growth at exactly 2000 clean steps
    assert got[3 + 2000 + 1999] == 1.0 and got[-2] == 1.0 and got[-1] == 2.0
    assert r.steps == len(pat) and r.skipped == 4 and r.since == 0
    pat = [0] * 4000
    got, r = _ref_run(pat, init_scale=32768.0)
    assert got == _host_run(32768.0, pat)
    assert got[1999] == 65536.0 and got[-1] == 65536.0              # the upper clamp, reached and held


def test_random_sequence_against_host_scaler():
    rng = np.random.default_rng(11)
    # overflows rare enough that runs of 2000 clean steps occur, frequent enough to reach 1
    pat = (rng.random(30000) < 4e-4).tolist()
    pat[100:120] = [True] * 20
    got, _ = _ref_run(pat, init_scale=1024.0)
    host = _host_run(1024.0, pat)
    assert got == host
    assert min(got) == 1.0 and max(got) > 1024.0 / 2 ** 10 and len(set(got)) > 3


def test_short_interval_variant():
    """growth_interval 3, scale 4 in [1, 16] (the device test's script): both clamps, by hand"""
    pat = [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0]
    got, r = _ref_run(pat, init_scale=4.0, growth_interval=3, min_scale=1.0, max_scale=16.0)
    assert got == [4, 4, 8, 8, 8, 16, 16, 16, 16, 8, 4, 2, 1, 1, 1, 1, 2]
    assert r.skipped == 5 and r.steps == 17 and r.since == 0
    # the unscale factor is the inverse of the scale the step's objective read, not the new one
    r = LossScaleRef(init_scale=8.0, growth_interval=1)
    assert r.update(False) is False and r.inv_used == np.float32(1 / 8) and r.scale == 16
    assert r.update(True) is True and r.inv_used == np.float32(1 / 16) and r.scale == 8
    r.set_scale(1e9)
    assert r.scale == 65536.0 and r.since == 0


def test_overflow_decision_reads_segments_only():
    g = np.ones(32, np.float32)
    segs = [(0, 5), (9, 20)]
    assert not overflow_of(g, segs)
    g[6] = np.inf                      # a gap
    g[3], g[10] = 3e38, 1e-45          # huge and subnormal are finite
    assert not overflow_of(g, segs)
    for bad in (np.inf, -np.inf, np.nan):
        h = g.copy()
        h[19] = bad
        assert overflow_of(h, segs)


def test_train_config_validation():
    from kfp16.trainer import TrainConfig
    assert TrainConfig().loss_scale == 0.0 and TrainConfig().loss_scale_growth_interval == 2000
    TrainConfig(loss_scale=65536.0, loss_scale_growth_interval=1)
    TrainConfig(natural_gradient=True)                      # without a loss scale: as before
    with pytest.raises(ValueError, match="natural_gradient"):
        TrainConfig(loss_scale=256.0, natural_gradient=True)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="loss_scale"):
            TrainConfig(loss_scale=bad)
    for bad in (0, -5):
        with pytest.raises(ValueError, match="growth_interval"):
            TrainConfig(loss_scale=4.0, loss_scale_growth_interval=bad)
