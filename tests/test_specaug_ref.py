"""SpecAugment without a device: the numpy restatement of the rule
(tests/specaug_ref.py) against the rule's own properties and statistics, and the xconfig keys
and the spec-augment entry points of kf_nnet.h on a layout-only net."""
import numpy as np
import pytest

import kfp16
from kfp16 import synth
from kfp16.trainer import TrainConfig

import dropout_ref as dr
import specaug_ref as sr

SA_LINE = "spec-augment-layer name=idct-spec-augment"


def _tiny(keys=""):
    x = synth.load_xconfig("tiny.xconfig")
    bn = "batchnorm-component name=idct-batchnorm input=idct\n"
    assert x.count(bn) == 1
    return x.replace(bn, bn + SA_LINE + (" " + keys if keys else "") + "\n")


def _runs(flags):
    """[(value, length)] of the runs of a boolean vector"""
    out = []
    for v in flags:
        if out and out[-1][0] == bool(v):
            out[-1][1] += 1
        else:
            out.append([bool(v), 1])
    return out


def test_derived_numbers():
    assert sr.max_bins(40, 0.5) == 20 and sr.max_bins(40, 0.0) == 0 and sr.max_bins(40, 1.0) == 40
    assert sr.max_bins(43, 0.5) == 22 and sr.max_bins(3, 0.1) == 0 and sr.max_bins(5, 0.1) == 1
    assert sr.max_kept(20, 0.2) == 80 and sr.max_kept(10, 0.2) == 40 and sr.max_kept(2, 0.5) == 2
    assert sr.max_kept(1, 0.9) == 1 and sr.max_kept(10, 0.0) == 1
    assert sr.max_kept(20, 1e-12) == 2 ** 31 - 1


def test_draw_is_the_philox_word():
    seed, step, k, b = 0x1234567890ABCDEF, 7, 3, 5
    for kind, i in ((0, 0), (0, 1), (1, 0), (1, 6), (1, 131)):
        want = dr.philox4x32_10(np.array([step, 0x80000000 | (2 * k + kind), b, i // 4], np.uint64),
                                np.array([0x90ABCDEF, 0x12345678], np.uint64))[i % 4]
        assert int(sr.draws(seed, step, k, b, kind, i, 1)[0]) == int(want)
    assert int(sr.randint(0xFFFFFFFF, 21)) == 20 and int(sr.randint(0, 21)) == 0
    assert int(sr.randint(0x80000000, 2 ** 31 - 1)) == 2 ** 30 - 1


@pytest.mark.parametrize("m,z", [(20, 0.2), (2, 0.5), (10, 0.0), (5, 0.9)])
def test_properties(m, z):
    D, f, seed = 40, 0.5, 99
    Z, m_n = sr.max_bins(D, f), sr.max_kept(m, z)
    so = [0, 1, 3, 66, 130, 195, 345, 1845, 1846]
    rows = sr.specaug_rows(seed, 3, 0, so, D, Z, z, m, m_n)
    assert rows.shape == (so[-1],) and rows.dtype == np.int32
    for b in range(len(so) - 1):
        seg = rows[so[b]:so[b + 1]]
        start, count = sr.band(seed, 3, 0, b, D, Z)
        assert 0 <= count <= Z and 0 <= start and start + count <= D
        kept = seg[seg != -1]
        assert np.all(kept == (start | (count << 16)))      # one band per sequence
        if z == 0:
            assert len(kept) == len(seg)                    # no row of -1
            continue
        runs = _runs(seg == -1)                             # regions alternate: runs are regions
        regs = sr.regions(seed, 3, 0, b, len(seg), z, m, m_n)
        assert [(zr, ln) for _, ln, zr in regs] == [(v, n) for v, n in runs]
        assert all(regs[i][2] != regs[i + 1][2] for i in range(len(regs) - 1))
        assert sum(ln for _, ln, _ in regs) == len(seg)
        for i, (v, n) in enumerate(runs):
            assert 1 <= n <= (m if v else m_n), (b, i, v, n)   # (a clipped last run is shorter still)


def test_no_band_and_every_coordinate_matters():
    so = [0, 150, 300]
    a = sr.specaug_rows(5, 0, 0, so, 40, 0, 0.2, 20, 80)
    assert np.all((a == -1) | (a >> 16 == 0))               # f = 0: count 0
    base = sr.specaug_rows(5, 0, 0, so, 40, 20, 0.2, 20, 80)
    assert not np.array_equal(base[:150], base[150:])       # sequences differ
    for kw in (dict(seed=6), dict(seed=5 + 2 ** 32), dict(step=1), dict(k=1)):
        args = dict(seed=5, step=0, k=0)
        args.update(kw)
        assert not np.array_equal(sr.specaug_rows(args["seed"], args["step"], args["k"], so, 40, 20, 0.2, 20, 80), base)


def test_statistics_at_the_fixed_seed():
    """seed 1234, step 0: 64 sequences of 150 frames, m = 20, z = 0.2 -> the zeroed share of
    frames in [0.15, 0.25] (a simulation of the rule over 200 seeds gave 0.171 ... 0.220), and
    the mean band width at D = 40, f = 0.5 in [7, 13] (uniform on 0 ... 20: mean 10)."""
    so = list(range(0, 64 * 150 + 1, 150))
    rows = sr.specaug_rows(1234, 0, 0, so, 40, sr.max_bins(40, 0.5), 0.2, 20, sr.max_kept(20, 0.2))
    share = float(np.mean(rows == -1))
    widths = [sr.band(1234, 0, 0, b, 40, 20)[1] for b in range(64)]
    print("zeroed share %.4f, mean band width %.3f" % (share, np.mean(widths)))
    assert 0.15 <= share <= 0.25
    assert 7 <= np.mean(widths) <= 13
    assert min(widths) >= 0 and max(widths) <= 20


def test_apply_is_a_select():
    x = np.array([[-1.0, np.nan, np.inf, 2.0, -0.0], [1.0, 2.0, 3.0, 4.0, 5.0], [np.nan, -np.inf, 1.0, 1.0, 1.0]], np.float16)
    rows = np.array([1 | (3 << 16), -1, 0], np.int32)       # band [1, 4), zeroed row, no band
    y = sr.specaug_apply(x, rows).view(np.uint16)
    xu = x.view(np.uint16)
    assert list(y[0]) == [xu[0, 0], 0, 0, 0, xu[0, 4]]
    assert list(y[1]) == [0] * 5
    assert np.array_equal(y[2], xu[2])


def test_xconfig_keys_and_layout_only_api():
    tiny = synth.load_xconfig("tiny.xconfig")
    net = kfp16.Network(tiny, 100, layout_only=True)
    assert net.spec_augment_layers() == []
    with pytest.raises(kfp16.KfError, match="not a spec-augment-layer"):
        net.spec_augment_opts("cnn1")
    net.set_spec_augment(True, 5)                          # no such layer: nothing to do
    net.close()

    # Kaldi's xconfig defaults; the layer adds no parameter and keeps its input's dim
    net = kfp16.Network(_tiny(), 100, layout_only=True)
    assert net.spec_augment_layers() == ["idct-spec-augment"]
    assert net.spec_augment_opts("idct-spec-augment") == (0.5, 0.2, 10)
    assert net.params.keys() == kfp16.Network(tiny, 100, layout_only=True).params.keys()
    assert [l for l in net.layers if l[0] == "idct-spec-augment"][0][2:] == (40, 40)
    net.close()
    assert "idct-spec-augment" in str(kfp16.parse_summary(_tiny()))

    net = kfp16.Network(_tiny("freq-max-proportion=0.25 time-zeroed-proportion=0.1 time-mask-max-frames=20"), 100,
                        layout_only=True)
    assert net.spec_augment_opts("idct-spec-augment") == (0.25, 0.1, 20)
    net.set_spec_augment_opts("idct-spec-augment", 1.0, 0.0, 1)
    assert net.spec_augment_opts("idct-spec-augment") == (1.0, 0.0, 1)
    for f, z, m in ((-0.1, 0.2, 10), (1.1, 0.2, 10), (0.5, -0.1, 10), (0.5, 1.0, 10), (0.5, 0.2, 0), (float("nan"), 0.2, 10),
                    (0.5, float("nan"), 10)):
        with pytest.raises(kfp16.KfError, match="set_spec_augment_opts"):
            net.set_spec_augment_opts("idct-spec-augment", f, z, m)
    assert net.spec_augment_opts("idct-spec-augment") == (1.0, 0.0, 1)
    with pytest.raises(kfp16.KfError, match="no layer"):
        net.set_spec_augment_opts("nope", 0.5, 0.2, 10)
    with pytest.raises(kfp16.KfError, match="not a spec-augment-layer"):
        net.set_spec_augment_opts("cnn1", 0.5, 0.2, 10)
    # the switch and the feature's own step need no device; the step is not dropout's
    net.set_spec_augment(True, seed=2 ** 63 + 5)
    assert net.spec_augment_step() == 0
    net.set_spec_augment_step(2 ** 32 - 1)
    assert net.spec_augment_step() == 2 ** 32 - 1 and net.dropout_step() == 0
    for bad in (-1, 2 ** 32):
        with pytest.raises(kfp16.KfError, match="step"):
            net.set_spec_augment_step(bad)
    net.set_spec_augment(False)
    with pytest.raises(kfp16.KfError, match="layout-only"):
        net.spec_augment_rows("idct-spec-augment")
    net.close()


def test_two_layers_get_ordinals_in_order():
    x = _tiny().replace("linear-component name=prefinal-l dim=64",
                        "spec-augment-layer name=sa2 time-mask-max-frames=3\nlinear-component name=prefinal-l dim=64")
    net = kfp16.Network(x, 100, layout_only=True)
    assert net.spec_augment_layers() == ["idct-spec-augment", "sa2"]
    assert net.spec_augment_opts("sa2") == (0.5, 0.2, 3)
    net.close()


@pytest.mark.parametrize("key,val", [("freq-max-proportion", "1.5"), ("freq-max-proportion", "-0.1"),
                                     ("freq-max-proportion", "abc"), ("freq-max-proportion", "nan"),
                                     ("time-zeroed-proportion", "1.0"), ("time-zeroed-proportion", "1"),
                                     ("time-zeroed-proportion", "-0.2"), ("time-zeroed-proportion", "0.2x"),
                                     ("time-mask-max-frames", "0"), ("time-mask-max-frames", "-3"),
                                     ("time-mask-max-frames", "2.5"), ("time-mask-max-frames", "ten")])
def test_xconfig_key_rejected(key, val):
    with pytest.raises(kfp16.KfError, match="idct-spec-augment.*" + key + ".*" + val):
        kfp16.parse_summary(_tiny(key + "=" + val))


def test_configs_and_train_config():
    cfg = TrainConfig()
    assert cfg.spec_augment is False and cfg.spec_augment_seed == 0
    assert TrainConfig(spec_augment=True, spec_augment_seed=9).spec_augment_seed == 9
    for name, m in (("specaug/tiny_specaug.xconfig", 10), ("specaug/tiny_ivec_specaug.xconfig", 10),
                    ("specaug/cnn_tdnn_17f_kaldi_specaug.xconfig", 20)):
        net = kfp16.Network(synth.load_xconfig(name), 100, layout_only=True)
        assert net.spec_augment_layers() == ["idct-spec-augment"]
        assert net.spec_augment_opts("idct-spec-augment") == (0.5, 0.2, m)
        net.close()
    # the layer changes nothing else of the net it was added to
    a = kfp16.Network(synth.load_xconfig("specaug/tiny_specaug.xconfig"), 100, layout_only=True)
    b = kfp16.Network(synth.load_xconfig("tiny.xconfig"), 100, layout_only=True)
    assert a.params == b.params and [l for l in a.layers if l[0] != "idct-spec-augment"] == b.layers
    a.close()
    b.close()
