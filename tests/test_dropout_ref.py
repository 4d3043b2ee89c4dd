"""Per-sequence dropout without a device: the numpy Philox4x32-10 against the
published known-answer vectors, the mask rule, Kaldi's dropout schedule, and the xconfig key
and the dropout entry points of kf_nnet.h on a layout-only net."""
import numpy as np
import pytest

import kfp16
from kfp16 import synth
from kfp16.trainer import dropout_proportion, parse_dropout_schedule

import dropout_ref as dr

TDNNF_KEY = "bypass-scale=0.66"


def _tiny_with_dropout(p="0.0"):
    x = synth.load_xconfig("tiny.xconfig")
    assert x.count(TDNNF_KEY) == 4
    return x.replace(TDNNF_KEY, TDNNF_KEY + " dropout-proportion=" + p)


# Random123 kat_vectors, "philox4x32 10": counter, key -> output
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = dr.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
    assert [int(v) for v in got] == want
    # batched form: the same block among others
    c = np.array([[1, 2, 3, 4], ctr, [9, 9, 9, 9]], np.uint64)
    assert [int(v) for v in dr.philox4x32_10(c, np.array(key, np.uint64))[1]] == want


def test_mask_rule():
    B, dim, p = 5, 64, 0.3
    m = dr.dropout_masks(seed=0x1234567890ABCDEF, step=7, ordinal=2, B=B, dim=dim, p=p)
    assert m.shape == (B, dim) and m.dtype == np.float32
    # uniform on [1 - 2p, 1 + 2p): inside the range, mean near 1 (320 draws: 5 sigma of 2p/sqrt(3)/sqrt(320))
    assert m.min() >= np.float32(1 - 2 * p) and m.max() < np.float32(1 + 2 * p) + 1e-6
    assert abs(float(m.mean()) - 1.0) < 5 * (2 * p / np.sqrt(3)) / np.sqrt(B * dim)
    # element (b, n) is word n % 4 of the block with counter (step, ordinal, b, n // 4), key = seed words
    b, n = 3, 37
    x = dr.philox4x32_10(np.array([7, 2, b, n // 4], np.uint64), np.array([0x90ABCDEF, 0x12345678], np.uint64))[n % 4]
    u = np.float32(int(x) >> 8) * np.float32(2.0 ** -24)
    assert m[b, n] == np.float32(np.float32(4 * p) * u + np.float32(1 - 2 * np.float32(p)))
    # every coordinate of the counter and the key matters; p = 0 is the identity; rows differ
    for kw in (dict(step=8), dict(ordinal=3), dict(seed=0x1234567890ABCDEE), dict(seed=0x0234567890ABCDEF)):
        args = dict(seed=0x1234567890ABCDEF, step=7, ordinal=2, B=B, dim=dim, p=p)
        args.update(kw)
        assert not np.array_equal(dr.dropout_masks(**args), m)
    assert np.all(dr.dropout_masks(1, 2, 3, B, dim, 0.0) == 1.0)
    assert not np.array_equal(m[0], m[1])


def test_row_segments():
    so = [0, 5, 37, 50]
    seg = dr.row_segments(so, 50)
    assert seg[0] == 0 and seg[4] == 0 and seg[5] == 1 and seg[36] == 1 and seg[37] == 2 and seg[49] == 2
    # compact rows: 3c for c < tc0, then the tail ... T-4, T-1
    T, tc0, tc = 50, 17, 19   # (T - 1) % 3 == 1: frames 46, 49 in the tail
    segc = dr.row_segments(so, T, tc0, tc)
    rows = [3 * c for c in range(tc0)] + [46, 49]
    assert list(segc) == [int(seg[r]) for r in rows]


def test_schedule_values():
    s = "0,0@0.20,0.5@0.50,0"
    got = [dropout_proportion(s, f) for f in (0, 0.1, 0.2, 0.35, 0.5, 0.75, 1)]
    assert got == pytest.approx([0, 0, 0, 0.25, 0.5, 0.25, 0], abs=1e-12)
    assert parse_dropout_schedule("0.1,0.3") == [(0.0, 0.1), (1.0, 0.3)]
    assert dropout_proportion("0.1,0.3", 0.5) == pytest.approx(0.2)
    assert dropout_proportion("0.1,0.3", -1) == pytest.approx(0.1) and dropout_proportion("0.1,0.3", 2) == pytest.approx(0.3)


@pytest.mark.parametrize("bad", ["", "0.3", "0,", "0,0.5@0.5", "0@0.1,0.2", "0,0.2,0", "0,0.2@0.5,0.3@0.5,0",
                                 "0,0.2@0.6,0.3@0.4,0", "0,0.2@1.0,0", "0,0.2@0,0", "0,0.6@0.5,0", "0,-0.1@0.5,0",
                                 "0,x@0.5,0", "0,0.2@0.5@0.6,0"])
def test_schedule_rejects(bad):
    with pytest.raises(ValueError):
        parse_dropout_schedule(bad)


def test_xconfig_key_and_layout_only_api():
    tiny = synth.load_xconfig("tiny.xconfig")
    net = kfp16.Network(tiny, 100, layout_only=True)
    assert net.dropout_layers() == []                      # default -1: no component
    assert net.dropout_proportion("tdnnf6") == -1.0
    net.set_dropout_proportion(0.2)                        # NULL layer: every layer with one (none)
    with pytest.raises(kfp16.KfError, match="no dropout component"):
        net.set_dropout_proportion(0.2, "tdnnf6")
    net.close()

    xd = _tiny_with_dropout("0.0")
    assert kfp16.parse_summary(xd) == kfp16.parse_summary(tiny)   # the key changes no shape
    net = kfp16.Network(xd, 100, layout_only=True)
    assert net.dropout_layers() == ["tdnnf5", "tdnnf6", "tdnnf7", "tdnnf8"]
    assert all(net.dropout_proportion(n) == 0.0 for n in net.dropout_layers())
    assert net.dropout_proportion("cnn1") == -1.0
    net.set_dropout_proportion(0.3)
    net.set_dropout_proportion(0.1, "tdnnf7")
    assert [round(net.dropout_proportion(n), 6) for n in net.dropout_layers()] == [0.3, 0.3, 0.1, 0.3]
    for p in (-0.1, 0.51, float("nan")):
        with pytest.raises(kfp16.KfError, match="proportion"):
            net.set_dropout_proportion(p)
    with pytest.raises(kfp16.KfError, match="no layer"):
        net.set_dropout_proportion(0.1, "nope")
    with pytest.raises(kfp16.KfError, match="no dropout component"):
        net.set_dropout_proportion(0.1, "cnn1")
    # the switch, the step and the sequence boundaries need no device
    net.set_dropout(True, seed=2 ** 63 + 5)
    assert net.dropout_step() == 0
    net.set_dropout_step(41)
    assert net.dropout_step() == 41
    with pytest.raises(kfp16.KfError):
        net.set_dropout_step(-1)
    net.set_sequences([0, 10, 50, 100])
    net.set_sequences(None)
    for bad in ([0, 10, 10, 100], [1, 10, 100], [0, 50, 101], [0]):
        with pytest.raises(kfp16.KfError, match="set_sequences"):
            net.set_sequences(bad)
    with pytest.raises(kfp16.KfError, match="layout-only"):
        net.dropout_mask("tdnnf6")
    net.close()

    # one layer with the key: only that layer is listed
    one = tiny.replace("name=tdnnf7 dim=256", "name=tdnnf7 dropout-proportion=0.25 dim=256")
    net = kfp16.Network(one, 100, layout_only=True)
    assert net.dropout_layers() == ["tdnnf7"] and net.dropout_proportion("tdnnf7") == 0.25
    net.close()


@pytest.mark.parametrize("val", ["0.6", "-0.5", "abc", "0.1x", "nan"])
def test_xconfig_key_rejected(val):
    with pytest.raises(kfp16.KfError, match="dropout-proportion.*" + val):
        kfp16.parse_summary(_tiny_with_dropout(val))


def test_xconfig_key_ignored_on_other_layers():
    tiny = synth.load_xconfig("tiny.xconfig")
    x = tiny.replace("name=prefinal-l dim=64", "name=prefinal-l dim=64 dropout-proportion=0.9")
    assert kfp16.parse_summary(x) == kfp16.parse_summary(tiny)
    net = kfp16.Network(x, 100, layout_only=True)
    assert net.dropout_layers() == []
    net.close()
