"""The update components of the Kaldi-style parameter update (kf_nnet.h nnet_update), on
layout-only networks (no GPU): names, tensor membership, xconfig options and their defaults,
the segments the kernel is given, nnet_set_component_opts and nnet_update_opts_from_kaldi.
"""
import os

import numpy as np
import pytest

import kfp16
from kfp16 import model, synth

T_CONV, T_TDNNF, T_LINEAR, T_PREFINAL, T_OUTPUT, T_ATT = 6, 7, 2, 9, 10, 8


def _expected(net):
    """[(component, tensors)] from the layer list, as kf_nnet.h states the grouping"""
    out = []
    for name, ty, _, _ in net.layers:
        if ty == T_CONV:
            out.append((name + ".conv", [name + ".W", name + ".Bias"]))
        elif ty == T_TDNNF:
            out.append((name + ".linear", [name + ".LinearW"]))
            out.append((name + ".affine", [name + ".AffineW", name + ".AffineBias"]))
        elif ty == T_LINEAR:
            out.append((name, [name + ".W"]))
        elif ty == T_PREFINAL:
            pre = "prefinal-xent" if "xent" in name else "prefinal-chain"
            out.append((pre + ".affine", [name + ".BigW", name + ".BigBias"]))
            out.append((pre + ".linear", [name + ".SmallW"]))
        elif ty in (T_OUTPUT, T_ATT):
            out.append((name + ".affine", [name + ".W", name + ".Bias"]))
    return out


@pytest.mark.parametrize("cfg", ["cnn_tdnn_17f.xconfig", "tiny.xconfig", "tiny_att.xconfig", "tiny_xent.xconfig"])
def test_components_names_tensors_defaults(cfg):
    net = kfp16.Network(synth.load_xconfig(cfg), max_frames=64, layout_only=True)
    comps = net.components()
    assert [(c["name"], c["tensors"]) for c in comps] == _expected(net)
    out_layers = {n for n, ty, _, _ in net.layers if ty == T_OUTPUT}
    assert out_layers
    for c in comps:
        is_out = c["name"].endswith(".affine") and c["name"][:-len(".affine")] in out_layers
        assert c["max_change"] == (1.5 if is_out else 0.75), c
        assert c["l2"] == 0.0 and c["lr_factor"] == 1.0, c
    # every tensor is in exactly one component
    owned = [t for c in comps for t in c["tensors"]]
    assert sorted(owned) == sorted(net.params)
    net.close()


def test_17f_has_the_named_components():
    net = kfp16.Network(synth.load_xconfig("cnn_tdnn_17f.xconfig"), max_frames=64, layout_only=True)
    by = {c["name"]: c for c in net.components()}
    for n in ("cnn1.conv", "tdnnf7.linear", "tdnnf7.affine", "prefinal-l", "prefinal-chain.affine",
              "prefinal-chain.linear", "output.affine"):
        assert n in by, n
    assert by["output.affine"]["max_change"] == 1.5
    assert by["tdnnf7.affine"]["tensors"] == ["tdnnf7.AffineW", "tdnnf7.AffineBias"]
    net.close()


def test_segments_exclude_padding_and_tile_the_buffer():
    """A component's segments are its tensors' rows * cols elements; with the 64-element
    alignment padding after each tensor they tile [0, num_params)."""
    net = kfp16.Network(synth.load_xconfig("cnn_tdnn_17f.xconfig"), max_frames=64, layout_only=True)
    segs = []
    for c in net.components():
        for t in c["tensors"]:
            r, k, off = net.params[t]
            segs.append((off, off + r * k))
    segs.sort()
    pos, padded = 0, 0
    for b, e in segs:
        assert b == pos and b % 64 == 0 and e > b
        pos = (e + 63) // 64 * 64
        padded += pos - e
    assert pos == net.num_params
    assert padded > 0                      # the layout has padding, and no segment covers it
    assert sum(e - b for b, e in segs) == net.num_params - padded
    net.close()


def _tiny_with(opts_cnn2, opts_tdnnf6):
    lines = []
    for ln in synth.load_xconfig("tiny.xconfig").splitlines():
        if "name=cnn2 " in ln:
            ln += " " + opts_cnn2
        if "name=tdnnf6 " in ln:
            ln += " " + opts_tdnnf6
        lines.append(ln)
    return "\n".join(lines) + "\n"


def test_xconfig_keys_reach_the_components():
    keys = "max-change=0.25 l2-regularize=0.01 learning-rate-factor=0.333"
    net = kfp16.Network(_tiny_with(keys, keys), max_frames=64, layout_only=True)
    by = {c["name"]: c for c in net.components()}
    want = (np.float32(0.25), np.float32(0.01), np.float32(0.333))
    for n in ("cnn2.conv", "tdnnf6.linear", "tdnnf6.affine"):
        assert (by[n]["max_change"], by[n]["l2"], by[n]["lr_factor"]) == want, n
    for n in ("cnn1.conv", "tdnnf5.linear", "tdnnf7.affine", "prefinal-l"):
        assert (by[n]["max_change"], by[n]["l2"], by[n]["lr_factor"]) == (0.75, 0.0, 1.0), n
    assert by["output.affine"]["max_change"] == 1.5
    net.close()


@pytest.mark.parametrize("bad, word", [("max-change=-1", "max-change"), ("learning-rate-factor=0", "learning-rate-factor"),
                                       ("l2-regularize=-0.5", "l2-regularize")])
def test_bad_option_values_are_parse_errors_with_the_line(bad, word):
    with pytest.raises(kfp16.KfError) as e:
        kfp16.Network(_tiny_with(bad, ""), max_frames=64, layout_only=True)
    assert word in str(e.value) and "line 6" in str(e.value) and "cnn2" in str(e.value), str(e.value)


def test_set_component_opts():
    net = kfp16.Network(synth.load_xconfig("tiny.xconfig"), max_frames=64, layout_only=True)
    before = net.components()
    net.set_component_opts("tdnnf7.affine", 0.5, 0.125, 2.0)
    after = {c["name"]: c for c in net.components()}
    assert (after["tdnnf7.affine"]["max_change"], after["tdnnf7.affine"]["l2"],
            after["tdnnf7.affine"]["lr_factor"]) == (0.5, 0.125, 2.0)
    assert [c for c in net.components() if c["name"] != "tdnnf7.affine"] == \
        [c for c in before if c["name"] != "tdnnf7.affine"]
    with pytest.raises(kfp16.KfError, match="no component tdnnf7.nothing"):
        net.set_component_opts("tdnnf7.nothing", 0.5)
    for args in ((-1.0, 0.0, 1.0), (0.5, -0.1, 1.0), (0.5, 0.0, 0.0), (float("nan"), 0.0, 1.0)):
        with pytest.raises(kfp16.KfError):
            net.set_component_opts("tdnnf7.affine", *args)
    assert {c["name"]: c for c in net.components()} == after   # a rejected call changes nothing
    net.set_component_opts("cnn1.conv", 0.0)                    # 0 = no limit is a valid value
    assert net.components()[0]["max_change"] == 0.0
    net.close()


def test_update_needs_device_storage():
    net = kfp16.Network(synth.load_xconfig("tiny.xconfig"), max_frames=64, layout_only=True)
    with pytest.raises(kfp16.KfError, match="layout-only"):
        net.update(1e-3, 0.9)
    net.close()


def _model_text(names, skip=()):
    """an nnet3 text model (the format of tests/golden/nnet3_*.txt) with one updatable
    component per name; max-change and l2 differ per component"""
    out, vals = [], {}
    for i, n in enumerate(names):
        if n in skip:
            continue
        mc, l2 = 0.5 + 0.125 * i, 0.001 * (i + 1)
        vals[n] = (np.float32(mc), np.float32(l2))
        out.append("<ComponentName> %s <NaturalGradientAffineComponent> <MaxChange> %g <L2Regularize> %g "
                   "<LearningRate> 0.0005 <LinearParams>  [\n  0.1 0.2\n  0.3 0.4 ]\n<BiasParams>  [ 0.5 0.6 ]\n"
                   % (n, mc, l2))
    return "".join(out), vals


def test_update_opts_from_kaldi():
    net = kfp16.Network(synth.load_xconfig("tiny.xconfig"), max_frames=64, layout_only=True)
    names = [c["name"] for c in net.components()]
    net.set_component_opts("tdnnf5.linear", 0.75, 0.0, 0.5)
    text, vals = _model_text(names)
    m = model.Nnet3Model.from_text(text)
    m.update_opts_into(net)
    for c in net.components():
        assert (c["max_change"], c["l2"]) == vals[c["name"]], c
        assert c["lr_factor"] == (0.5 if c["name"] == "tdnnf5.linear" else 1.0)  # not taken from the model
    m.close()
    # a model without one of the components: an error that leaves every option as it was
    before = net.components()
    text2, _ = _model_text(list(reversed(names)), skip=("tdnnf8.affine",))
    m2 = model.Nnet3Model.from_text(text2)
    with pytest.raises(model.ModelError, match="tdnnf8.affine not found"):
        m2.update_opts_into(net)
    assert net.components() == before
    m2.close()
    net.close()
