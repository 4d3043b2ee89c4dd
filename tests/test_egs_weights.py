"""The weights a batch of egs carries (kf_egs_batch_weights, kf_egs_batch_deriv_weights;
TrainingBatch.example_weights / deriv_weights()) on the CPU: each example's
<Weight>, its <DW2> / <DW> per-frame deriv weights, ones where an example has no block, the
errors, and that the batch itself assembles as before."""
import numpy as np
import pytest

import egs_writer as W
from kfp16 import egs, trainer

FPS = 13


def _parts(rng):
    return (W.random_matrix(rng, "CM", 100, 40), W.random_matrix(rng, "CM2", 1, 100),
            [W.random_num_fst(rng, int(n)) for n in (10, 7, 12)])


def _batch(tmp_path, name, examples):
    W.write_ark(tmp_path / name, examples)
    b = egs.DataLoader(str(tmp_path / name), batch_size=len(examples)).next_batch()
    assert b is not None and b.batch_size == len(examples)
    return b


def _check_layout(b, feats, states, keys):
    """batch_size, offsets and CSR from the writer's metadata alone"""
    B = len(states)
    assert b.batch_size == B and b.keys == keys
    rows = feats[1]["rows"]
    assert b.num_frames.tolist() == [rows] * B and b.frame_offsets.tolist() == [rows * i for i in range(B)]
    assert b.total_frames == rows * B and b.frames_per_seq.tolist() == [FPS] * B
    ns = [len(s) for s in states]
    na = [sum(len(a) for a, _ in s) for s in states]
    assert b.state_offsets.tolist() == np.concatenate([[0], np.cumsum(ns)[:-1]]).tolist()
    assert b.per_seq["state_off"].tolist() == np.concatenate([[0], np.cumsum(ns)]).tolist()
    assert b.per_seq["arc_off"].tolist() == np.concatenate([[0], np.cumsum(na)]).tolist()
    assert b.csr["num_states"] == sum(ns) and b.csr["num_arcs"] == sum(na)
    rp, col, lab, logw, off = [0], [], [], [], 0
    for s in states:
        for arcs, _ in s:
            col += [n + off for (_, _, n) in arcs]
            lab += [l for (l, _, _) in arcs]
            logw += [-np.float32(w) for (_, w, _) in arcs]
            rp.append(len(col))
        off += len(s)
    assert b.csr["row_ptr"].tolist() == rp and b.csr["col"].tolist() == col and b.csr["label"].tolist() == lab
    assert np.array_equal(b.csr["logw"], np.asarray(logw, np.float32))
    assert b.csr["final_state"].tolist() == (np.cumsum(ns) - 1).tolist()
    for i, s in enumerate(states):
        f = b.num_fsts()[i]
        assert f["S"] == len(s) and f["row_ptr"].tolist() == np.concatenate([[0], np.cumsum([len(a) for a, _ in s])]).tolist()
        assert f["dst"].tolist() == [n for a, _ in s for (_, _, n) in a]
    assert b.num_sequences == 1


def test_batch_weight_accessors(tmp_path):
    rng = np.random.default_rng(17)
    feats, ivec, st = _parts(rng)
    dw = np.array([0, 0.25, 0.5, 1], np.float32)[rng.integers(0, 4, FPS)]
    dwb = rng.uniform(0, 1, FPS).astype(np.float32)
    exs = [W.example_bytes("utt-a", feats, ivec, fst_states=st[0], frames_per_seq=FPS, deriv_weights=dw),
           W.example_bytes("utt-b", feats, ivec, fst_states=st[1], frames_per_seq=FPS, deriv_weights=dwb, dw_kind="DW"),
           W.example_bytes("utt-c", feats, ivec, fst_states=st[2], frames_per_seq=FPS, weight=0.5)]
    b = _batch(tmp_path, "w.ark", exs)
    assert b.example_weights.dtype == np.float32 and b.example_weights.tolist() == [1.0, 1.0, 0.5]
    assert b.weight == 1.0                                   # the first example's, as before
    got, have = b.deriv_weights()
    q = np.clip(np.round(dwb * 255), 0, 255).astype(np.uint8)
    want = np.concatenate([dw, q.astype(np.float32) / np.float32(255.0), np.ones(FPS, np.float32)])
    assert have is True and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _check_layout(b, feats, st, ["utt-a", "utt-b", "utt-c"])


def test_batch_without_any_block_gives_ones(tmp_path):
    rng = np.random.default_rng(18)
    feats, ivec, st = _parts(rng)
    exs = [W.example_bytes(f"utt-{i}", feats, ivec, fst_states=st[i], frames_per_seq=FPS, weight=w)
           for i, w in enumerate((2.0, 1.0, 0.25))]
    b = _batch(tmp_path, "n.ark", exs)
    got, have = b.deriv_weights()
    assert have is False and np.array_equal(got, np.ones(3 * FPS, np.float32))
    assert b.example_weights.tolist() == [2.0, 1.0, 0.25] and b.weight == 2.0
    _check_layout(b, feats, st, ["utt-0", "utt-1", "utt-2"])


def test_wrong_count_and_several_sequences_are_errors(tmp_path):
    rng = np.random.default_rng(19)
    feats, ivec, st = _parts(rng)
    ok = W.example_bytes("utt-ok", feats, ivec, fst_states=st[0], frames_per_seq=FPS)
    short = W.example_bytes("utt-short", feats, ivec, fst_states=st[1], frames_per_seq=FPS,
                            deriv_weights=np.ones(FPS - 1, np.float32))
    b = _batch(tmp_path, "s.ark", [ok, short])
    with pytest.raises(egs.EgsError, match=r"utt-short.*12 deriv weights.*13"):
        b.deriv_weights()
    assert b.example_weights.tolist() == [1.0, 1.0]          # the batch itself assembled as before
    _check_layout(b, feats, st[:2], ["utt-ok", "utt-short"])
    two = W.example_bytes("utt-two", feats, ivec, fst_states=st[2], frames_per_seq=FPS, num_sequences=2,
                          deriv_weights=np.ones(FPS, np.float32))
    b2 = _batch(tmp_path, "t.ark", [ok, two])
    with pytest.raises(egs.EgsError, match=r"utt-two.*num_sequences=2"):
        b2.deriv_weights()
    plain2 = W.example_bytes("utt-two", feats, ivec, fst_states=st[2], frames_per_seq=FPS, num_sequences=2)
    got, have = _batch(tmp_path, "u.ark", [ok, plain2]).deriv_weights()   # no weights: no error
    assert have is False and np.all(got == 1.0)


def test_train_config_defaults_are_off():
    cfg = trainer.TrainConfig()
    assert cfg.apply_deriv_weights is False and cfg.example_weights is False
