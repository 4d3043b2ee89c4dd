"""The self-repair rule's reference (tests/self_repair_ref.py) and the xconfig keys;
no device."""
import os

import numpy as np
import pytest

import bn_train_ref as br
import self_repair_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(rows=37, D=16, seed=3):
    rng = np.random.default_rng(seed)
    r = np.maximum(rng.standard_normal((rows, D)) + 0.3, 0.0).astype(np.float16).astype(np.float64)
    g = (rng.standard_normal((rows, D)) * 0.1).astype(np.float16).astype(np.float64)
    f = br.bn_train_forward(r, br.EPS, 0.75)
    return r, g, f, (r > 0).astype(np.uint8)


def test_zero_scale_is_the_batchnorm_backward():
    r, g, f, bits = _case()
    s = sr.repair_vector(37.0, sr.relu_counts(r), 0.0)
    assert not s.any()
    a, b, dz = sr.repair_backward(g, r, f["scale"], f["shift"], 0.75, bits, s)
    a0, b0, gr0 = br.bn_train_backward(g, r, f["scale"], f["shift"], 0.75)
    assert np.array_equal(a, a0) and np.array_equal(b, b0) and np.array_equal(dz, gr0 * bits)


def test_rows_form_leaves_the_tail_rows_alone():
    r, g, f, bits = _case()
    s = np.full(16, 2.0 ** -10, np.float32)
    _, _, dz = sr.repair_backward(g, r, f["scale"], f["shift"], 0.75, bits, s, stat_rows=30)
    _, _, dz0 = sr.repair_backward(g, r, f["scale"], f["shift"], 0.75, bits, 0 * s, stat_rows=30)
    assert np.array_equal(dz[30:], dz0[30:])
    assert np.array_equal(dz[:30], dz0[:30] + 2.0 ** -10)


def test_thresholds_on_exact_products():
    """lower = 0.25, upper = 0.75, count = 20: every product is exact in double. Equality is dead,
    equality is not saturated."""
    k = 2.0 ** -10
    s = sr.repair_vector(20.0, [5, 6, 15, 16, 0, 20, 10], k, 0.25, 0.75)
    assert s.dtype == np.float32
    assert s.tolist() == [-k, 0.0, 0.0, k, -k, k, 0.0]
    assert not sr.repair_vector(0.0, [0, 0, 5], k, 0.25, 0.75).any()
    s = sr.repair_vector(20.0, [5, 16], 1e-5, 0.25, 0.75, S=4096.0)
    assert s.tolist() == [-float(np.float32(1e-5) * np.float32(4096)), float(np.float32(1e-5) * np.float32(4096))]


def test_counts_per_column_and_per_block():
    r = np.zeros((3, 8))
    r[:, 1] = 1.0
    r[1, 2] = 0.5
    assert sr.relu_counts(r).tolist() == [0, 3, 1, 0, 0, 0, 0, 0]
    assert sr.relu_counts(r, H=2).tolist() == [0, 3, 1, 0]     # block f = columns f and 4 + f


def test_one_sgd_step_raises_a_dead_bias_and_lowers_a_saturated_one():
    rows, D, k = 20, 8, 2.0 ** -10
    rng = np.random.default_rng(5)
    r = np.maximum(rng.standard_normal((rows, D)), 0.0)
    r[:, 0] = 0.0          # dead
    r[:, 1] = 1.0 + rng.random(rows)  # saturated
    g = np.zeros((rows, D))
    f = br.bn_train_forward(r, br.EPS, 1.0)
    bits = (r > 0).astype(np.uint8)
    s = sr.repair_vector(rows, sr.relu_counts(r), k)
    assert s[0] == -np.float32(k) and s[1] == np.float32(k)
    _, _, dz = sr.repair_backward(g, r, f["scale"], f["shift"], 1.0, bits, s)
    bias_grad = dz.sum(0)            # the affine's bias gradient is dz's column sum
    bias = np.zeros(D)
    new = sr.sgd_step(bias, bias_grad, 0.1)
    assert new[0] > bias[0] and new[1] < bias[1]
    assert bias_grad[0] == -k * rows and bias_grad[1] == k * rows


def test_tdnnf_response_matches_finite_differences():
    """the clamped splices' transposes: d/dW of sum_t s . (affine output) at random W"""
    rng = np.random.default_rng(9)
    T, din, bn, dout, st = 11, 4, 3, 5, 3
    x = rng.standard_normal((T, din)).astype(np.float16).astype(np.float64)
    W1, W2 = rng.standard_normal((2 * din, bn)) * 0.25, rng.standard_normal((2 * bn, dout)) * 0.25
    s = rng.standard_normal(dout).astype(np.float16).astype(np.float64)
    t = np.arange(T)
    lo, hi = np.maximum(t - st, 0), np.minimum(t + st, T - 1)

    def loss(W1, W2):
        bott = np.concatenate([x[lo], x], 1) @ W1
        return float((np.concatenate([bott, bott[hi]], 1) @ W2 @ s).sum())

    got = sr.tdnnf_response(x, W1, W2, s, st)
    num = np.zeros_like(W1)
    for i in range(W1.shape[0]):
        for j in range(W1.shape[1]):
            d = np.zeros_like(W1)
            d[i, j] = 1e-3
            num[i, j] = (loss(W1 + d, W2) - loss(W1 - d, W2)) / 2e-3
    # (the reference rounds the bottleneck to fp16 for the affine's gradient only; the loss is
    # linear in W1, so the central difference is exact up to rounding)
    assert np.allclose(got["LinearW"], num, rtol=1e-9, atol=1e-9)
    assert np.allclose(got["AffineBias"], T * s)


def _xcfg(extra_tdnnf="", extra_conv="", extra_prefinal=""):
    text = open(os.path.join(ROOT, "configs", "tiny.xconfig")).read()
    text = text.replace("name=tdnnf6 ", "name=tdnnf6 " + extra_tdnnf + " ")
    text = text.replace("name=cnn2 ", "name=cnn2 " + extra_conv + " ")
    return text.replace("name=prefinal-chain ", "name=prefinal-chain " + extra_prefinal + " ")


def test_xconfig_keys():
    import kfp16
    net = kfp16.Network(_xcfg("self-repair-scale=0.001 self-repair-lower-threshold=0.25", "self-repair-upper-threshold=0.75",
                              "self-repair-scale=0"), max_frames=30, layout_only=True)
    o = net.self_repair_opts("tdnnf6")
    assert o["scale"] == float(np.float32(0.001)) and o["lower"] == 0.25 and o["upper"] == 0.95
    o = net.self_repair_opts("cnn2")
    assert o["scale"] == float(np.float32(1e-5)) and o["lower"] == 0.05 and o["upper"] == 0.75
    assert net.self_repair_opts("prefinal-chain")["scale"] == 0.0
    assert net.self_repair_opts("tdnnf5") == {"scale": float(np.float32(1e-5)), "lower": 0.05, "upper": 0.95}
    with pytest.raises(kfp16.KfError, match="no ReLU that self-repair applies to"):
        net.self_repair_opts("output")
    net.set_self_repair_opts("tdnnf5", 2.0 ** -10, 0.25, 0.75)
    assert net.self_repair_opts("tdnnf5") == {"scale": 2.0 ** -10, "lower": 0.25, "upper": 0.75}
    for bad in ((-1.0, 0.05, 0.95), (1e-5, 0.5, 0.5), (1e-5, -0.1, 0.9), (1e-5, 0.1, 1.5)):
        with pytest.raises(kfp16.KfError, match="set_self_repair_opts"):
            net.set_self_repair_opts("tdnnf5", *bad)
    net.close()


@pytest.mark.parametrize("bad", ["self-repair-scale=-1e-5", "self-repair-scale=abc", "self-repair-lower-threshold=-0.1",
                                 "self-repair-upper-threshold=1.5", "self-repair-lower-threshold=0.96",
                                 "self-repair-lower-threshold=0.5 self-repair-upper-threshold=0.5"])
def test_xconfig_bad_values_fail_at_parse(bad):
    import kfp16
    with pytest.raises(kfp16.KfError, match="self-repair"):
        kfp16.Network(_xcfg(bad), max_frames=30, layout_only=True)
    with pytest.raises(kfp16.KfError, match="self-repair"):
        kfp16.Network(_xcfg("", bad), max_frames=30, layout_only=True)


def test_existing_configs_parse_as_before():
    import kfp16
    for name in ("tiny.xconfig", "cnn_tdnn_17f_kaldi.xconfig"):
        net = kfp16.Network(open(os.path.join(ROOT, "configs", name)).read(), max_frames=30, layout_only=True)
        net.close()


def test_staged_oracle_adds_the_term_after_the_relu_bit():
    """SelfRepairOracle: a zero term is BnSitesOracle's backward exactly; with a term, a dead unit's
    bias gradient (ReLU bit 0 on every row, which the oracle's own backward would multiply in) is
    rne_fp16(s) n, n H for a conv filter, and the parameters above a site do not move"""
    import kfp16
    from kfp16 import synth
    import bn_sites_ref as bs
    T = 48
    xcfg = synth.load_xconfig("tiny.xconfig")
    net = kfp16.Network(xcfg, max_frames=T, layout_only=True)
    params = synth.make_params(net.params, seed=42)
    conv_fout, prefinal = synth.layer_dims(net)
    bns = synth.make_bn_all(synth.bn_specs(net.layers, conv_fout, prefinal))
    net.close()
    dead = {"tdnnf6": ("tdnnf6.AffineBias", 256, 1), "cnn2": ("cnn2.Bias", 32, 20), "prefinal-chain": ("prefinal-chain.BigBias", 256, 1)}
    for pname, _, _ in dead.values():
        params[pname] = params[pname].copy()
        params[pname][0, 3] = -30.0
    tp = {k: synth.trunc_fp16(v) for k, v in params.items()}
    feats = synth.make_features(T, 40, seed=1234).astype(np.float32)
    og = (np.random.default_rng(7).standard_normal((T, 200)) * 0.05).astype(np.float16).astype(np.float32)
    sites = ["tdnnf", "conv", "prefinal"]
    base = bs.BnSitesOracle(xcfg, tp, bns, sites, threads=8)
    base.forward(feats)
    want = base.backward(og)
    base.close()
    k = 2.0 ** -10
    repair = {}
    for layer, (_, D, _) in dead.items():
        repair[layer] = np.zeros(D, np.float32)
    zero = sr.SelfRepairOracle(xcfg, tp, bns, sites, threads=8, repair=repair)
    zero.forward(feats)
    got = zero.backward(og)
    zero.close()
    assert set(got) == set(want) and all(np.array_equal(got[n], want[n]) for n in want)
    for layer in dead:
        repair[layer][3] = -k
    ref = sr.SelfRepairOracle(xcfg, tp, bns, sites, threads=8, repair=repair)
    ref.forward(feats)
    assert all(not ref.masks[layer].reshape(-1, D)[:, 3].any() for layer, (_, D, _) in dead.items())
    got = ref.backward(og)
    ref.close()
    for layer, (pname, D, H) in dead.items():
        assert want[pname].reshape(-1)[3] == 0.0
        assert abs(got[pname].reshape(-1)[3] + k * T * H) <= 1e-6 * k * T * H, (layer, got[pname].reshape(-1)[3])
    assert np.array_equal(got["output.W"], want["output.W"]) and np.array_equal(got["prefinal-chain.SmallW"], want["prefinal-chain.SmallW"])
    assert not np.array_equal(got["tdnnf5.LinearW"], want["tdnnf5.LinearW"])      # the layers below a site see the term
