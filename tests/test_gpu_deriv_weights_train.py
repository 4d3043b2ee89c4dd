"""EgsTrainer with TrainConfig.apply_deriv_weights / example_weights on
configs/tiny_xent.xconfig: six egs of the writer fixture (rows 150, 183, 129 twice, P = 200) that
carry <DW2> and <DW> deriv weights, one without a block, per-eg <Weight>s, and one eg whose
supervision is cut short by its input (40 frames asked, 33 fit: it keeps its first 33 weights).
learning_rate = 0: the step's gradients are what is under test.

Every comparison is bit for bit: the same kernels run with the same weights, whether the
trainer hands them over or the test does; the row-subsampled step's output rows are those of
the all-rows step (tests/test_gpu_row_subsampling.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 200
XR = 0.1
ROWS = (150, 183, 129, 150, 183, 129)
EG_WEIGHTS = (1.0, 0.5, 2.0, 1.0, 0.25, 1.0)


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    import egs_writer as W
    from kfp16 import egs, synth, trainer
    rng = np.random.default_rng(31)
    exs, dws = [], []
    for e, R in enumerate(ROWS):
        fps = 40 if e == 5 else (R - 60) // 3
        if e == 2:
            dw, kind = None, "DW2"
        elif e == 1:
            dw, kind = rng.uniform(0, 1, fps).astype(np.float32), "DW"
        elif e == 3:
            dw, kind = np.array([0, 0.25, 0.5, 1], np.float32)[rng.integers(0, 4, fps)], "DW2"
        else:
            dw, kind = np.linspace(0.1, 1.0, fps).astype(np.float32), "DW2"
        exs.append(W.example_bytes(f"utt-{e:04d}", W.random_matrix(rng, "CM", R, 40), W.random_matrix(rng, "CM2", 1, 100),
                                   fst_states=W.random_num_fst(rng, int(rng.integers(8, 21)), P), frames_per_seq=fps,
                                   weight=EG_WEIGHTS[e], deriv_weights=dw, dw_kind=kind))
        if dw is None:
            dws.append(np.ones(fps, np.float32))
        elif kind == "DW":
            dws.append(np.clip(np.round(dw * 255), 0, 255).astype(np.uint8).astype(np.float32) / np.float32(255.0))
        else:
            dws.append(dw)
    d = tmp_path_factory.mktemp("dw")
    W.write_ark(d / "cegs.1.ark", exs)
    batch = egs.DataLoader(str(d / "cegs.*.ark"), batch_size=6).next_batch()
    den = synth.make_den_graph(num_states=300, num_arcs=3000, num_pdfs=P)
    row0, frames = trainer.chain_rows(batch.frame_offsets, batch.num_frames, batch.frames_per_seq, 3, 30)
    assert frames.tolist() == [30, 41, 23, 30, 41, 33] and batch.frames_per_seq[5] == 40
    assert np.all(row0 % 3 == 0)
    # what the objective must get: each eg's first frames[i] weights
    frame_w = np.concatenate([w[:n] for w, n in zip(dws, frames)])
    return dict(batch=batch, den=den, row0=row0, frames=frames, frame_w=frame_w,
                seq_w=np.asarray(EG_WEIGHTS, np.float32))


def _trainer(gpu, fx, **kw):
    from kfp16 import synth, trainer
    cfg = trainer.TrainConfig(learning_rate=0.0, momentum=0.0, xent_regularize=XR, **kw)
    tr = trainer.EgsTrainer(synth.load_xconfig("tiny_xent.xconfig"), fx["den"], max_egs=8, max_frames=1200, config=cfg)
    synth.init_network(tr.net)
    return tr


def _outputs(gpu, tr, rows):
    gpu.sync()
    return dict(grad=gpu.read_fp16(tr.grad_out.ptr, (rows, P)), xgrad=gpu.read_fp16(tr.xent_grad.ptr, (rows, P)),
                wgrads=tr.net.read_grads())


def _by_hand(gpu, tr, fx, seq_w, frame_w):
    """the step of a trainer with the options off, the weights handed to Chain.compute here"""
    from kfp16 import chain
    batch, T = fx["batch"], fx["batch"].total_frames
    batch.features_to_device(tr.feat.ptr, 40)
    tr._zero_grads(T)
    tr.net.forward(tr.feat.ptr, T)
    nb = chain.NumBatch(batch.num_fsts())
    tr.objective.compute(nb, tr.out_ptr, P, T, fx["row0"], fx["frames"], 3, tr.grad_out.ptr, P, tr.opts,
                         seq_weight=seq_w, frame_weight=frame_w)
    tr.objective.xent(nb, tr.xent_ptr, P, tr.xent_grad.ptr, P, tr.opts)
    tr.net.backward(tr.grad_out.ptr, tr.xent_grad.ptr)
    out = _outputs(gpu, tr, T)
    out["res"] = tr.result()
    nb.close()
    return out


def _equal(a, b):
    for k in ("grad", "xgrad"):
        np.testing.assert_array_equal(a[k].view(np.uint16), b[k].view(np.uint16), err_msg=k)
    assert a["wgrads"].keys() == b["wgrads"].keys()
    for k, v in a["wgrads"].items():
        np.testing.assert_array_equal(v.view(np.uint32), b["wgrads"][k].view(np.uint32), err_msg=k)


@pytest.fixture(scope="module")
def plain(gpu, fixture):
    """the unweighted all-rows step (a trainer built without the new fields)"""
    tr = _trainer(gpu, fixture)
    tr.step(fixture["batch"])
    out = _outputs(gpu, tr, fixture["batch"].total_frames)
    out["res"] = tr.result()
    tr.net.close()
    return out


@pytest.fixture(scope="module")
def weighted(gpu, fixture):
    """the all-rows step with both options on"""
    tr = _trainer(gpu, fixture, apply_deriv_weights=True, example_weights=True)
    tr.step(fixture["batch"])
    out = _outputs(gpu, tr, fixture["batch"].total_frames)
    out["res"] = tr.result()
    tr.net.close()
    return out


def test_options_against_hand_weighted_objective(gpu, fixture, plain, weighted):
    """grad_out, the xent gradient and every weight gradient of the step with the options on are
    those of a step with the options off whose objective got the same weights by hand; both
    differ from the unweighted step; no statistic but the weight depends on them."""
    fx = fixture
    tr = _trainer(gpu, fx)
    hand = _by_hand(gpu, tr, fx, fx["seq_w"], fx["frame_w"])
    tr.net.close()
    _equal(weighted, hand)
    sup0 = fx["row0"][0] + 3 * np.arange(fx["frames"][0])
    for k in ("grad", "xgrad"):
        assert np.any(weighted[k][sup0] != plain[k][sup0]), k
        assert np.any(weighted[k][sup0]), k
    assert any(np.any(weighted["wgrads"][k] != plain["wgrads"][k]) for k in plain["wgrads"])
    r, h, p = weighted["res"], hand["res"], plain["res"]
    assert (r.objf, r.total_weight, r.xent_objf, r.xent_weight) == (h.objf, h.total_weight, h.xent_objf, h.xent_weight)
    assert r.num_ok == 6 and r.frames == p.frames == int(fx["frames"].sum())
    assert r.total_weight == float(np.sum(fx["seq_w"].astype(np.float64) * fx["frames"])) != p.total_weight
    assert r.num_logprob == p.num_logprob and r.den_logprob == p.den_logprob


@pytest.mark.parametrize("which", ["apply_deriv_weights", "example_weights"])
def test_each_option_alone(gpu, fixture, plain, which):
    """one option on: the step of the other weight as ones"""
    fx = fixture
    tr = _trainer(gpu, fx, **{which: True})
    tr.step(fx["batch"])
    got = _outputs(gpu, tr, fx["batch"].total_frames)
    tr.net.close()
    tr = _trainer(gpu, fx)
    hand = _by_hand(gpu, tr, fx, *((None, fx["frame_w"]) if which == "apply_deriv_weights" else (fx["seq_w"], None)))
    tr.net.close()
    _equal(got, hand)
    assert np.any(got["grad"] != plain["grad"])


def test_row_subsampled_step_holds_the_same_weighted_rows(gpu, fixture, weighted):
    """row_subsampling: the step takes the compact path, and on the supervised rows the
    compact-row grad_out and xent gradient are the all-rows step's weighted rows."""
    fx = fixture
    tr = _trainer(gpu, fx, apply_deriv_weights=True, example_weights=True, row_subsampling=True)
    tr.step(fx["batch"])
    r = tr.result()
    tc, _tc0, rows = tr.net.row_set()
    assert tr.full_row_steps == 0 and tc > 0
    got = _outputs(gpu, tr, tc)
    tr.net.close()
    sup = np.concatenate([r0 + 3 * np.arange(n) for r0, n in zip(fx["row0"], fx["frames"])])
    assert np.array_equal(np.asarray(rows)[sup // 3], sup)          # compact row c is frame 3c
    for k in ("grad", "xgrad"):
        np.testing.assert_array_equal(got[k][sup // 3].view(np.uint16), weighted[k][sup].view(np.uint16), err_msg=k)
        rest = np.ones(tc, bool)
        rest[sup // 3] = False
        assert not np.any(got[k][rest]), k
    w = weighted["res"]
    assert (r.objf, r.total_weight, r.xent_objf) == (w.objf, w.total_weight, w.xent_objf)


def test_options_off_is_the_step_as_before(gpu, fixture, plain):
    """both fields False explicitly: bit-identical to a trainer built without them, although the
    egs carry weights"""
    tr = _trainer(gpu, fixture, apply_deriv_weights=False, example_weights=False)
    tr.step(fixture["batch"])
    got = _outputs(gpu, tr, fixture["batch"].total_frames)
    r = tr.result()
    tr.net.close()
    _equal(got, plain)
    p = plain["res"]
    assert (r.objf, r.total_weight, r.xent_objf) == (p.objf, p.total_weight, p.xent_objf)
    assert r.total_weight == float(fixture["frames"].sum())
