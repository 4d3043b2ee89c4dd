"""The orthonormal-constraint value of the update components (kf_nnet.h
nnet_component_orthonormal / nnet_set_component_orthonormal), on layout-only networks (no
GPU): xconfig defaults per layer kind, explicit keys, parse errors, setter errors and what
nnet_update_opts_from_kaldi carries over.
"""
import numpy as np
import pytest

import kfp16
from kfp16 import model, synth


def _layout(xcfg):
    return kfp16.Network(xcfg, max_frames=64, layout_only=True)


def _values(net):
    return {c["name"]: net.component_orthonormal(c["name"]) for c in net.components()}


def _with(name, keys, cfg="tiny.xconfig"):
    lines = []
    for ln in synth.load_xconfig(cfg).splitlines():
        if f"name={name} " in ln:
            ln += " " + keys
        lines.append(ln)
    return "\n".join(lines) + "\n"


def test_defaults_on_tiny():
    net = _layout(synth.load_xconfig("tiny.xconfig"))
    v = _values(net)
    constrained = ["tdnnf5.linear", "tdnnf6.linear", "tdnnf7.linear", "tdnnf8.linear", "prefinal-chain.linear"]
    assert net.orthonormal_components() == constrained
    for name, c in v.items():
        assert c == (-1.0 if name in constrained else 0.0), name
    assert v["prefinal-l"] == 0.0
    net.close()


def test_defaults_on_17f_kaldi():
    net = _layout(synth.load_xconfig("cnn_tdnn_17f_kaldi.xconfig"))
    v = _values(net)
    tdnnf = [n for n in v if n.startswith("tdnnf") and n.endswith(".linear")]
    prefinal = [n for n in v if n.startswith("prefinal-") and n.endswith(".linear")]
    assert len(tdnnf) == 17 and sorted(prefinal) == ["prefinal-chain.linear", "prefinal-xent.linear"]
    for name, c in v.items():
        assert c == (-1.0 if name in tdnnf + prefinal else 0.0), name
    assert v["prefinal-l"] == 0.0 and v["ivector-linear"] == 0.0
    assert all(not n.endswith(".affine") or c == 0.0 for n, c in v.items())
    assert len(net.orthonormal_components()) == 19
    net.close()


def test_explicit_keys():
    net = _layout(_with("tdnnf6", "orthonormal-constraint=0.5"))
    v = _values(net)
    assert v["tdnnf6.linear"] == 0.5 and v["tdnnf6.affine"] == 0.0 and v["tdnnf5.linear"] == -1.0
    net.close()
    net = _layout(_with("prefinal-l", "orthonormal-constraint=-1"))
    assert _values(net)["prefinal-l"] == -1.0
    assert "prefinal-l" in net.orthonormal_components()
    net.close()
    net = _layout(_with("tdnnf7", "orthonormal-constraint=0"))
    assert _values(net)["tdnnf7.linear"] == 0.0 and "tdnnf7.linear" not in net.orthonormal_components()
    net.close()
    # on a layer kind the key does not apply to it is not read, like any unknown key
    net = _layout(_with("cnn2", "orthonormal-constraint=-1"))
    assert _values(net)["cnn2.conv"] == 0.0
    net.close()


@pytest.mark.parametrize("bad", ["abc", "nan", "inf", "", "1x"])
def test_bad_value_is_a_parse_error_with_the_line(bad):
    xcfg = _with("tdnnf6", "orthonormal-constraint=" + bad)
    line = 1 + [i for i, ln in enumerate(xcfg.splitlines()) if "name=tdnnf6 " in ln][0]
    with pytest.raises(kfp16.KfError) as e:
        _layout(xcfg)
    assert "orthonormal-constraint" in str(e.value) and f"line {line}" in str(e.value) and "tdnnf6" in str(e.value)


def test_setter_and_its_errors():
    net = _layout(synth.load_xconfig("cnn_tdnn_17f_kaldi.xconfig"))
    before = _values(net)
    net.set_component_orthonormal("tdnnf8.linear", 0.75)
    net.set_component_orthonormal("prefinal-l", -1.0)
    net.set_component_orthonormal("tdnnf9.linear", 0.0)
    after = _values(net)
    assert (after["tdnnf8.linear"], after["prefinal-l"], after["tdnnf9.linear"]) == (0.75, -1.0, 0.0)
    assert {k: v for k, v in after.items() if k not in ("tdnnf8.linear", "prefinal-l", "tdnnf9.linear")} == \
        {k: v for k, v in before.items() if k not in ("tdnnf8.linear", "prefinal-l", "tdnnf9.linear")}
    with pytest.raises(kfp16.KfError, match="no component tdnnf8.nothing"):
        net.set_component_orthonormal("tdnnf8.nothing", -1.0)
    with pytest.raises(kfp16.KfError, match="not a single weight matrix"):
        net.set_component_orthonormal("tdnnf8.affine", -1.0)            # carries a bias
    with pytest.raises(kfp16.KfError, match="transposed case not supported"):
        net.set_component_orthonormal("ivector-linear", -1.0)           # 100 -> 200: n > K
    with pytest.raises(kfp16.KfError):
        net.set_component_orthonormal("tdnnf8.linear", float("nan"))
    net.set_component_orthonormal("ivector-linear", 0.0)                # off is valid on any single matrix
    assert _values(net) == after                                        # a rejected call changes nothing
    with pytest.raises(kfp16.KfError, match="layout-only"):
        net.constrain_orthonormal()
    net.close()


def _model_text(net, tags):
    """an nnet3 text model (the format of tests/golden/nnet3_*.txt) with one component per
    update component of net; tags: {name: text put on the component's header line}"""
    out = []
    for c in net.components():
        n = c["name"]
        kind = "TdnnComponent" if n.startswith("tdnnf") else "LinearComponent" if c["tensors"][0].endswith(
            ("SmallW", ".W")) and len(c["tensors"]) == 1 else "NaturalGradientAffineComponent"
        out.append("<ComponentName> %s <%s> <MaxChange> 0.75 <L2Regularize> 0.001 %s <LearningRate> 0.0005 "
                   "<LinearParams>  [\n  0.1 0.2\n  0.3 0.4 ]\n<BiasParams>  [ 0.5 0.6 ]\n" % (n, kind, tags.get(n, "")))
    return "".join(out)


def test_import_carries_a_present_tag_only():
    net = _layout(synth.load_xconfig("tiny.xconfig"))
    net.set_component_orthonormal("tdnnf5.linear", 0.25)
    before = _values(net)
    # no tag anywhere: the values stay
    m = model.Nnet3Model.from_text(_model_text(net, {}))
    assert m.orthonormal_constraint("tdnnf6.linear") is None
    m.update_opts_into(net)
    assert _values(net) == before
    assert all(c["l2"] == np.float32(0.001) for c in net.components())   # the other options were taken
    m.close()
    # present tags are taken: a floating one, a fixed one, an off one, and Kaldi's 0 on the
    # bias-carrying TdnnComponent (nothing to set there)
    tags = {"tdnnf5.linear": "<OrthonormalConstraint> -1", "tdnnf6.linear": "<OrthonormalConstraint> 0.5",
            "tdnnf7.linear": "<OrthonormalConstraint> 0", "tdnnf7.affine": "<OrthonormalConstraint> 0",
            "prefinal-l": "<OrthonormalConstraint> -1"}
    m = model.Nnet3Model.from_text(_model_text(net, tags))
    assert m.orthonormal_constraint("tdnnf6.linear") == 0.5 and m.orthonormal_constraint("tdnnf8.linear") is None
    m.update_opts_into(net)
    want = dict(before)
    want.update({"tdnnf5.linear": -1.0, "tdnnf6.linear": 0.5, "tdnnf7.linear": 0.0, "prefinal-l": -1.0})
    assert _values(net) == want
    m.close()
    # a value the component cannot take: an error that changes nothing
    m = model.Nnet3Model.from_text(_model_text(net, {"tdnnf8.affine": "<OrthonormalConstraint> -1",
                                                     "tdnnf8.linear": "<OrthonormalConstraint> 0"}))
    with pytest.raises(model.ModelError, match="tdnnf8.affine"):
        m.update_opts_into(net)
    assert _values(net) == want
    m.close()
    net.close()
