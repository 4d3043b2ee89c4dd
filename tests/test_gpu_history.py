"""History independence: a step's result depends on its inputs and switches, not on what the net ran
before. One net (one Chain) is taken through changing T and sequence counts (§1), through switches
flipped between steps (§2) and through weights that change under the copies derived from them (§3);
every compared step is bit-identical (np.array_equal on the unsigned views, history_dev.same) to
the same step run first on a fresh net. The fresh nets are anchored where no other test runs them
(§4: small T against the CPU oracle, the row set's edges against full rows), the Chain object keeps
nothing of an earlier layout (§5), and no switch grows the net when it is set again (§6).

Before every compared step the live net runs the previous step's shape again on other features at
four times the amplitude (Live.disturb), so whatever stays in rows beyond the new T, in the shared
ring slots or in cached tables is unrelated data. The dropout and SpecAugment generators are pinned
immediately before every forward, on both nets.

The only tolerances are §4's: the project's oracle bars (2e-3 relative Frobenius and 1e-2 of the
largest value on activations, 5e-3 on gradients) and test_gpu_row_subsampling.py's 1e-5 on the
gradients a compact run sums in another split-K order."""
import numpy as np
import pytest
import torch  # noqa: F401  (the HIP runtime first: the libraries then bind the same copy)

import history_dev as hd
from conftest import max_abs_rel, rel_fro
from history_dev import DROPOUT, IMPLICIT, NATGRAD, SPECAUG, WGRAD, Recipe, bn_train, fp8, fresh, rsub, same

pytestmark = pytest.mark.gpu

SEQS = {300: (0, 90, 200, 300), 149: (0, 149), 200: (0, 40, 80, 120, 160, 200)}
RSUB_T = [300, 298, 299, 131, 128, 46, 43, 300]
NT3 = 7            # tiny3 / tiny3c: three 3-strided layers above cnn4, + 4
NT_XENT = 5        # tiny_xent: one


def _walk(kf, recipe, Ts, nt=None, seqs=False, check_counts=False, **kw):
    """one net of the recipe through Ts; every step against a fresh net at that T"""
    live = recipe.make(kf)
    prev = None
    try:
        for T in Ts:
            seq = SEQS[T] if seqs else None
            want = hd.expected_row_set(T, nt) if nt is not None else (0, 0)
            if prev is not None:
                live.disturb(prev, seq=SEQS[prev] if seqs else None, **{k: v for k, v in kw.items() if k == "two_seeds"})
            before = live.bn_counts() if check_counts else None
            got = live.step(T, seq=seq, want_rows=want, **kw)
            ref = fresh(kf, recipe, T, seq=seq, want_rows=want, **kw)
            same(got, ref, "%s T=%d after %s" % (recipe.key, T, prev))
            if check_counts:
                # the accumulators grow by design: by exactly the rows this forward contributed
                after = live.bn_counts()
                assert after and all(after[k] - before[k] == live.bn_rows(k, T) for k in after), (T, before, after)
            prev = T
    finally:
        live.close()


# ---------------------------------------------------------------------------
# §1 varying T and sequence count on one net
# ---------------------------------------------------------------------------
def test_plain_varying_T(gpu):
    """10 frames: below one row tile and below four times the time stride"""
    _walk(gpu, Recipe("tiny"), [300, 149, 10, 300])


@pytest.mark.parametrize("cfg,conv", [("tiny3", None), ("tiny3", "0"), ("tiny3c", None), ("tiny3c", "0"), ("tiny3w", None)])
def test_row_subsampling_varying_T(gpu, cfg, conv):
    """compact rows with a tail at every residue of (T - 1) % 3 (300: 2, 299: 1; 298: none), the
    smallest T with a tail (131: tc0 = 44 = 4 * 7 + 16) and without one (46: tc0 = 16), the fall back
    to full rows one below each (128, 43), and 300 again after the row-mask cache has seen four other
    shapes. tiny3's cnn4 subsamples the height, so it never runs on the compact rows and KF_RSUB_CONV
    changes nothing there; tiny3c's cnn5 does (asserted); tiny3w's cnn4 would, but its weight
    gradient over the compact rows has no kernel, so the setter leaves it on full rows (before this
    was checked there, that net's backward failed with kf_gemm_wgrad's "time-strided rows")."""
    kf = gpu
    recipe = Recipe(cfg, rsub(conv))
    live = recipe.make(kf)
    live.step(300, backward=False)
    tc = live.net.row_set()[0]
    conv_rows = live.net.read_activation(hd.top_conv(cfg)).shape[0]
    assert tc == 107 and conv_rows == (tc if (cfg, conv) == ("tiny3c", None) else 300)
    live.close()
    _walk(kf, recipe, RSUB_T, nt=NT3)


@pytest.mark.parametrize("sw", [IMPLICIT, fp8(1), fp8(2)], ids=lambda s: s.name)
def test_implicit_dz_and_mxfp8_varying_T(gpu, sw):
    _walk(gpu, Recipe("tiny", sw), [300, 149, 300])


@pytest.mark.parametrize("sub", [False, True], ids=["full-rows", "row-subsampling"])
def test_dropout_varying_sequences(gpu, sub):
    """B = 3, 1, 5, 3: drop_B changes, the compact row -> sequence map is rebuilt"""
    recipe = Recipe("tiny3d", rsub(), DROPOUT) if sub else Recipe("tiny3d", DROPOUT)
    _walk(gpu, recipe, [300, 149, 200, 300], nt=NT3 if sub else None, seqs=True)


@pytest.mark.parametrize("sub", [False, True], ids=["rows-all", "rows-subsampled"])
@pytest.mark.parametrize("sites", ["tdnnf", "all"])
def test_batchnorm_train_varying_T(gpu, sites, sub):
    """the batch statistics are part of the snapshot; the accumulators' count grows by the rows of
    each step (the rows c < tc0 of a compact layer, every (block) row elsewhere)"""
    recipe = Recipe("tiny3", rsub(), bn_train(sites, "subsampled")) if sub else Recipe("tiny3", bn_train(sites, "all"))
    _walk(gpu, recipe, [300, 131, 298, 300], nt=NT3 if sub else None, check_counts=True)


def test_specaug_varying_sequences(gpu):
    _walk(gpu, Recipe("specaug", SPECAUG), [300, 149, 300], seqs=True)


def test_ivector_varying_sequences(gpu):
    """nnet_forward_ivector with B = 3, 1, 5, 3 and new ivectors each time: the per-sequence branch
    (rows < B) and the per-sequence gradient gdb are in the snapshot"""
    _walk(gpu, Recipe("tiny_ivec"), [300, 149, 200, 300], seqs=True)


def test_attention_varying_T(gpu):
    _walk(gpu, Recipe("tiny_att"), [300, 149, 300])


def test_two_seed_backward_varying_T(gpu):
    _walk(gpu, Recipe("tiny_xent"), [300, 149, 300], two_seeds=True)


CAPACITY = {"plain": (Recipe("tiny"), None), "rsub": (Recipe("tiny3", rsub()), NT3),
            "rsub-conv": (Recipe("tiny3c", rsub()), NT3),
            "bn": (Recipe("tiny3", rsub(), bn_train("tdnnf", "subsampled")), NT3)}


@pytest.mark.parametrize("T", [131, 300])
@pytest.mark.parametrize("mode", sorted(CAPACITY))
def test_capacity_is_not_read(gpu, mode, T):
    """a fresh net of max_frames = T against a fresh net of max_frames = 300"""
    recipe, nt = CAPACITY[mode]
    want = hd.expected_row_set(T, nt, max_frames=T) if nt else (0, 0)
    assert want == (hd.expected_row_set(T, nt) if nt else (0, 0))
    same(fresh(gpu, recipe, T, max_frames=T, want_rows=want), fresh(gpu, recipe, T, want_rows=want), "%s T=%d" % (mode, T))


# ---------------------------------------------------------------------------
# §2 switching modes on a live net
# ---------------------------------------------------------------------------
# id -> (xconfig, switches on throughout, the switch, sequences given)
SWITCHES = {
    "fp8-1": ("tiny", (), fp8(1), False), "fp8-2": ("tiny", (), fp8(2), False),
    "implicit-dz": ("tiny", (), IMPLICIT, False),
    "rsub": ("tiny3", (), rsub(), False), "rsub-conv": ("tiny3c", (), rsub(), False),
    "dropout": ("tiny3d", (), DROPOUT, True), "specaug": ("specaug", (), SPECAUG, True),
    "bn-tdnnf": ("tiny", (), bn_train("tdnnf"), False), "bn-conv": ("tiny", (), bn_train("conv"), False),
    "bn-prefinal": ("tiny", (), bn_train("prefinal"), False), "bn-batchnorm": ("tiny", (), bn_train("batchnorm"), False),
    "bn-all": ("tiny", (), bn_train("all"), False),
    "bn-rows": ("tiny3", (rsub(),), bn_train("tdnnf", "subsampled"), False),
    "one-stream": ("tiny", (), WGRAD, False), "natgrad": ("tiny", (), NATGRAD, False),
}


def _rows_of(cfg, recipe):
    on = any(s.name.startswith("rsub") for s in recipe.switches)
    return hd.expected_row_set(300, NT_XENT if cfg == "xent3d" else NT3, on)


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_switch_off_and_on_again(gpu, name):
    """(a) on, a step at 149 frames, off: the step at 300 is that of a net that never had the switch
    on; on again: the first step of a net that has it on (3 -> 0 -> 3 for row subsampling;
    nnet_set_natural_gradient starts the preconditioners again)"""
    kf = gpu
    cfg, base, sw, seqs = SWITCHES[name]
    off, on = Recipe(cfg, *base), Recipe(cfg, *base).plus(sw)
    seq = SEQS[300] if seqs else None
    live = on.make(kf)
    live.disturb(149, seq=SEQS[149] if seqs else None)
    live.switch(sw, False)
    same(live.step(300, seq=seq, want_rows=_rows_of(cfg, off)), fresh(kf, off, 300, seq=seq), name + ": off after on")
    live.disturb(149, seq=SEQS[149] if seqs else None)
    live.switch(sw, True)
    same(live.step(300, seq=seq, want_rows=_rows_of(cfg, on)), fresh(kf, on, 300, seq=seq), name + ": on again")
    live.close()


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_switch_on_late(gpu, name):
    """(b) a step with the switch off, then on: the first step of a net that had it on from the start"""
    kf = gpu
    cfg, base, sw, seqs = SWITCHES[name]
    off, on = Recipe(cfg, *base), Recipe(cfg, *base).plus(sw)
    seq = SEQS[300] if seqs else None
    live = off.make(kf)
    live.disturb(149, seq=SEQS[149] if seqs else None)
    live.switch(sw, True)
    same(live.step(300, seq=seq, want_rows=_rows_of(cfg, on)), fresh(kf, on, 300, seq=seq), name + ": on after off")
    live.close()


@pytest.mark.parametrize("first,second", [(None, "0"), ("0", None)], ids=["conv-to-gather", "gather-to-conv"])
def test_rsub_conv_changes_across_two_setter_calls(gpu, first, second):
    """KF_RSUB_CONV 1 -> 0 (and back) across two nnet_set_row_subsampling(3) calls on one net of
    tiny3c: cnn5 on the compact rows, then on full rows and read gathered"""
    kf = gpu
    live = Recipe("tiny3c", rsub(first)).make(kf)
    live.disturb(149)
    live.switch(rsub(second))
    got = live.step(300, want_rows=(107, 100))
    assert got["act/cnn5"].shape[0] == (107 if second is None else 300)
    same(got, fresh(kf, Recipe("tiny3c", rsub(second)), 300), "KF_RSUB_CONV %s -> %s" % (first, second))
    live.close()


def test_xent_seed_switches(gpu):
    """a two-seed backward at 149 frames, then a one-seed one at 300: a fresh net's (the branch's
    gradients exactly zero again); and the other way round (gx made late)"""
    kf = gpu
    r = Recipe("tiny_xent")
    for two in (False, True):
        live = r.make(kf)
        live.disturb(149, two_seeds=not two)
        got = live.step(300, two_seeds=two)
        same(got, fresh(kf, r, 300, two_seeds=two), "two_seeds=%s after %s" % (two, not two))
        branch = [k for k in got if k.startswith(("grad/prefinal-xent.", "grad/output-xent."))]
        assert branch and all(np.any(got[k]) == two for k in branch)
        live.close()


# the combinations kConflicts (host/modes.cpp) admits and no other test runs together
COMBOS = {
    "dropout-natgrad": ("tiny3d", [DROPOUT, NATGRAD], True, False),
    "specaug-bn-rsub": ("specaug3", [SPECAUG, rsub(), bn_train("tdnnf", "subsampled")], True, False),
    "dropout-two-seeds-rsub": ("xent3d", [DROPOUT, rsub()], True, True),
}


@pytest.mark.parametrize("name", sorted(COMBOS))
def test_admitted_combinations_in_either_order(gpu, name):
    """the modes switched on in the order A, B and in the order B, A: one step each, bit-identical;
    the row set is the one the rule gives, so none of them is a silent fall back"""
    kf = gpu
    cfg, sws, seqs, two = COMBOS[name]
    snaps = []
    for order in (sws, sws[::-1]):
        live = Recipe(cfg).make(kf)
        for sw in order:
            live.switch(sw)
        snaps.append(live.step(300, seq=SEQS[300] if seqs else None, two_seeds=two, want_rows=_rows_of(cfg, Recipe(cfg, *sws))))
        live.close()
    same(snaps[0], snaps[1], name)
    if name != "dropout-natgrad":
        assert snaps[0]["rows"][0] > 0


def _backward_n(net):
    import kfp16 as kf
    gb = kf.upload_fp16(hd.out_grad(300))
    kf.check(kf.nnet.nnet_backward_n(net.h, gb.ptr, 2), "nnet_backward_n")


def _backward_xent(net):
    import kfp16 as kf
    gb = kf.upload_fp16(hd.out_grad(300))
    net.backward(gb.ptr, gb.ptr)


BACKWARD_N = hd.Switch("backward_n", _backward_n, None)
BACKWARD_XENT = hd.Switch("backward_xent", _backward_xent, None)
# the pairs the table refuses (data parallel needs several processes: not here). A call, not a
# switch, as the second: one order only.
REFUSED = [("tiny", fp8(1), NATGRAD), ("tiny3d", fp8(1), DROPOUT), ("tiny", fp8(1), bn_train()), ("sa2", fp8(1), SPECAUG),
           ("tiny3d", IMPLICIT, DROPOUT), ("tiny", IMPLICIT, bn_train()), ("tiny3", rsub(), bn_train()),
           ("tiny", NATGRAD, BACKWARD_N), ("tiny3d", DROPOUT, BACKWARD_N), ("tiny", bn_train(), BACKWARD_N),
           ("tiny_xent", fp8(1), BACKWARD_XENT)]


@pytest.mark.parametrize("cfg,a,b", REFUSED, ids=lambda v: v if isinstance(v, str) else v.name)
def test_refused_pairs_leave_the_state_unchanged(gpu, cfg, a, b):
    """refused in both orders; the step after the refusal is the step before it"""
    kf = gpu
    seq = SEQS[300] if cfg in ("tiny3d", "sa2") else None
    for x, y in ((a, b), (b, a)):
        if x.off is None:
            continue
        back = cfg != "sa2"    # (no gradient passes a spec-augment layer that lies above a trainable one)
        # the step before it as a net takes it that was never asked: its second step (the natural
        # gradient's preconditioners move with every backward, so a step there does not replay)
        ref = Recipe(cfg, x).make(kf)
        ref.step(300, seq=seq, backward=back)
        want = ref.step(300, seq=seq, backward=back)
        ref.close()
        live = Recipe(cfg, x).make(kf)
        live.step(300, seq=seq, backward=back)
        with pytest.raises(kf.KfError, match="not supported|MXFP8 copy"):
            live.switch(y)
        same(live.step(300, seq=seq, backward=back), want, "%s: %s refused beside %s" % (cfg, y.name, x.name))
        live.close()


# ---------------------------------------------------------------------------
# §3 weights changing under derived copies
# ---------------------------------------------------------------------------
def _new_bns(live):
    from kfp16 import synth
    conv_fout, prefinal = synth.layer_dims(live.net)
    return synth.make_bn_all(synth.bn_specs(live.net.layers, conv_fout, prefinal), seed=45)


def _set_bns(net, bns):
    for (name, which), (m, v, g, b) in bns.items():
        net.set_bn(name, which, m, v, g, b, eps=1e-3)


def _accumulate_and_commit(live):
    """one training-mode forward, then nnet_bn_commit; MXFP8 and implicit dz, which refuse the mode,
    are off meanwhile"""
    held = list(live.on.values())
    for s in held:
        live.switch(s, False)
    sw = bn_train("tdnnf,conv,prefinal")
    live.switch(sw)
    live.step(300, seq=SEQS[300] if live.ivec else None, backward=False)
    live.switch(sw, False)
    assert live.net.batchnorm_commit() > 0
    for s in held:
        live.switch(s)


def _mutate(live, how):
    """-> what the fresh net is given besides the weights (the mutators that move BatchNorm)"""
    from kfp16 import model, synth
    import nnet3_writer as NW
    net = live.net
    if how == "set_params":
        net.set_params(synth.make_params(net.params, seed=77, bias_seed=78))
    elif how == "sgd":
        net.sgd(1e-3, 0.9)
    elif how == "update":
        net.update(1e-3, 0.9, 2.0, 100.0)
    elif how == "constrain_orthonormal":
        assert net.orthonormal_components()
        net.constrain_orthonormal()
    elif how == "load_into":
        bns = _new_bns(live)
        text = NW.network_text(net.layers, synth.make_params(net.params, seed=77, bias_seed=78), bns)
        assert model.Nnet3Model.from_text(text).load_into(net, model.LOAD_NEW).params > 0
        return lambda c: _set_bns(c.net, bns)
    elif how == "set_bn":
        bns = _new_bns(live)
        _set_bns(net, bns)
        return lambda c: _set_bns(c.net, bns)
    elif how == "batchnorm_commit":
        _accumulate_and_commit(live)
        # (the committed statistics have no getter: the fresh net accumulates and commits the same
        # forward itself, before it is given the weights; nothing of that forward reads them later)
        return _accumulate_and_commit
    return lambda c: None


MUTATORS = ["set_params", "sgd", "update", "constrain_orthonormal", "load_into", "set_bn", "batchnorm_commit"]
WEIGHT_NETS = {"tiny": Recipe("tiny"), "tiny-fp8": Recipe("tiny", fp8(1)), "tiny-implicit": Recipe("tiny", IMPLICIT),
               "ivec-im2col": Recipe("tiny_ivec")}


# (the nnet3 text fixture, nnet3_writer.network_text, writes tiny's layer kinds: no ivector branch)
WEIGHT_CASES = [(w, m) for w in sorted(WEIGHT_NETS) for m in MUTATORS if (w, m) != ("ivec-im2col", "load_into")]


@pytest.mark.parametrize("which,how", WEIGHT_CASES)
def test_weights_change_under_derived_copies(gpu, which, how):
    """Net A has run a step, so its transposed copies (wt), MXFP8 copies (w8, w8b, w8d), padded conv
    weights (wpad) and transposed conv taps (wtd) exist and hold the old weights; then one mutator,
    then the compared step. Net C is fresh and is given A's fp16 weights and masters device to
    device, then nnet_weights_changed. tiny_ivec's cnn1 (6 input filters: not 1, not a multiple of
    32) takes the im2col path. nnet_weights_changed on A and the step again changes nothing."""
    kf = gpu
    recipe = WEIGHT_NETS[which]
    seq = SEQS[300] if which == "ivec-im2col" else None
    a = recipe.make(kf)
    a.disturb(200 if seq else 211, seq=SEQS[200] if seq else None)
    also = _mutate(a, how)
    got = a.step(300, seq=seq)
    c = recipe.make(kf)
    also(c)
    n = a.net.num_params
    kf.check(kf.core.ops_copy(kf.nnet.nnet_weight_buffer(c.net.h), kf.nnet.nnet_weight_buffer(a.net.h), n), "copy fp16 weights")
    kf.check(kf.core.ops_copy(c.net.master_ptr, a.net.master_ptr, 2 * n), "copy masters")
    c.net.weights_changed()
    same(got, c.step(300, seq=seq), "%s after %s" % (which, how))
    c.close()
    unchanged = fresh(kf, recipe, 300, seq=seq)
    assert hd.differ(got, unchanged), "the mutator changed nothing"
    a.net.weights_changed()
    same(a.step(300, seq=seq), got, "%s: weights_changed after %s" % (which, how))
    if how == "update":
        st = a.net.update_stats()
        assert np.isfinite(st["global_norm"]) and st["global_norm"] > 0
    a.close()


# ---------------------------------------------------------------------------
# §4 reference anchors for the shapes no other test runs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [10, 46])
def test_small_T_against_the_oracle(gpu, T):
    """tiny at 10 and 46 frames (max_frames 300, as the fresh nets of §1) against oracle.OracleNet
    in its fused rounding mode, at test_tiny_network_forward_backward's bars; the share of equal
    ReLU decisions is not asserted (a few thousand bits a layer: two near-zero pre-activations
    would exceed 1 - 0.999), the disagreeing bits are printed.
    Measured: T=10 activations 7.0e-4 / 7.2e-4, gradients 7.5e-4 (cnn1.W), 0 of 51200 bits disagree;
    T=46 activations 7.2e-4 / 9.6e-4, gradients 1.1e-3 (cnn1.Bias), 3 of 235520 bits."""
    import oracle
    from kfp16 import synth
    kf = gpu
    live = Recipe("tiny").make(kf)
    net = live.net
    feats = hd.features(T)
    fb = kf.upload_fp16(feats)
    net.forward(fb.ptr, T)
    tp = {k: synth.trunc_fp16(v) for k, v in live.params.items()}
    on = oracle.OracleNet(live.xcfg, tp, live.bns, round_mode=oracle.ROUND_FUSED, threads=16)
    on.forward(feats.astype(np.float32))
    masks = net.relu_masks()
    worst, flips = (0.0, 0.0), 0
    for name, *_ in net.layers:
        got, ref = net.read_activation(name).astype(np.float32), on.act(name)
        e = (rel_fro(got, ref), max_abs_rel(got, ref))
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
        assert e[0] <= 2e-3 and e[1] <= 1e-2, (name, e)
        if name in masks:
            flips += int(np.sum(masks[name] != on.mask(name)))
    on.close()
    on = oracle.OracleNet(live.xcfg, tp, live.bns, round_mode=oracle.ROUND_FUSED, threads=16)
    on.forward(feats.astype(np.float32), force_masks=masks)
    og = (np.random.default_rng(7).standard_normal((T, 200)) * 0.05).astype(np.float16)
    gb = kf.upload_fp16(og)
    net.backward(gb.ptr)
    got = net.read_grads()
    on.backward(og.astype(np.float32))
    ref = on.grads()
    on.close()
    errs = {k: rel_fro(got[k], ref[k]) for k in ref}
    print("T=%d: activations %.2e rel-Frobenius, %.2e of the largest value; %d of %d ReLU bits disagree; "
          "gradients %.2e (%s)" % (T, worst[0], worst[1], flips, sum(m.size for m in masks.values()),
                                    max(errs.values()), max(errs, key=errs.get)))
    assert set(errs) == set(got)
    bad = {k: v for k, v in errs.items() if v > 5e-3}
    assert not bad, bad
    live.close()


@pytest.mark.parametrize("T", [299, 131, 46])
@pytest.mark.parametrize("cfg", ["tiny3", "tiny3c"])
def test_row_set_edges_against_full_rows(gpu, cfg, T):
    """the compact run against the full-row run of the same net, as
    test_row_subsampled_step_matches_full: rows c < tc0 of the output and of the inner activations
    bit-identical to rows 3c, the conv gradients bit-identical (but those of a conv that ran on the
    compact rows itself: tiny3c's cnn5), the others within 1e-5 relative Frobenius.
    Measured, the largest per T: tiny3 1.3e-7 (299, prefinal-l.W), 1.0e-7 (131, tdnnf7.LinearW), 5.3e-8
    (46, tdnnf5.LinearW); tiny3c 1.9e-7, 1.8e-7, 1.1e-7 (cnn5.W each): fifty times inside the bar."""
    kf = gpu
    want = hd.expected_row_set(T, NT3)
    assert want[0] > 0
    full = fresh(kf, Recipe(cfg), T)
    sub = fresh(kf, Recipe(cfg, rsub()), T, want_rows=want)
    tc, tc0 = want
    compact_conv = cfg == "tiny3c"
    conv = hd.top_conv(cfg)
    assert sub["act/" + conv].shape[0] == (tc if compact_conv else T)
    for k in ("act/output", "act/tdnnf6"):
        assert sub[k].shape[0] == tc
        assert np.array_equal(sub[k][:tc0].view(np.uint16), full[k][:3 * tc0:3].view(np.uint16)), k
    c4 = sub["act/" + conv]
    assert np.array_equal((c4[:tc0] if compact_conv else c4[::3]).view(np.uint16), full["act/" + conv][::3].view(np.uint16))
    worst = {}
    for k in [k for k in full if k.startswith("grad/")]:
        if k.startswith(("grad/cnn", "grad/idct")) and not (compact_conv and k.startswith("grad/" + conv)):
            assert np.array_equal(sub[k].view(np.uint32), full[k].view(np.uint32)), k
        else:
            worst[k] = rel_fro(sub[k], full[k])
    print("%s T=%d: largest %.2e (%s)" % (cfg, T, max(worst.values()), max(worst, key=worst.get)))
    bad = {k: v for k, v in worst.items() if v > 1e-5}
    assert not bad, bad


# ---------------------------------------------------------------------------
# §5 the Chain object
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_chain_keeps_nothing_of_an_earlier_layout(gpu, weighted):
    """one Chain on L1 (3 sequences, stride 3), L2 (1 sequence of another length, compact rows),
    L3 (5 sequences of unequal length) and L1 again: objective, statistics, gradients and xent
    gradients of every compute bit-identical to a fresh Chain's; the rows outside the layout keep
    the sentinel.

    All but one statistic: a sequence's l2_term (statistic 3, and KfChainResult.l2_term, their sum)
    is added up by k_den_post with a float atomicAdd per two-frame block (chain_den.hip, "if (do_l2
    && ok) atomicAdd(&st8[3], ...)"), so its last bit follows the order in which a sequence's blocks
    arrive, on a fresh Chain as on a used one (measured: 1 or 2 of the 12 statistics of the weighted
    run differ by one ulp from run to run, the first compute of two new Chains among them). It is
    printed, not compared; no gradient reads it."""
    import chain_ref as cr
    from kfp16 import chain as kc
    from test_gpu_chain_weights import _Run, _case, _res_tuple
    kf = gpu
    c = _case(200)
    layouts = [((0, 1, 2), 3), ((1,), 1), ((1, 0, 2, 0, 1), 3), ((0, 1, 2), 3)]

    def pair():
        dg = kc.DenGraph(c.g, c.init)
        return dg, kc.Chain(dg, max_seqs=5, max_frames=9)

    def weights(r, seed):
        if not weighted:
            return {}
        rng = np.random.default_rng(seed)
        n = int(r.frames.sum())
        return dict(seq_weight=rng.uniform(0.5, 2.0, len(r.frames)).astype(np.float32),
                    frame_weight=rng.uniform(0.1, 1.0, n).astype(np.float32))

    live = pair()
    l2_bits = 0
    for i, (seqs, stride) in enumerate(layouts):
        r = _Run(kf, c, stride, seqs=seqs, chain=live)
        got = r.run(**weights(r, 40 + i))
        one = pair()
        f = _Run(kf, c, stride, seqs=seqs, chain=one)
        want = f.run(**weights(f, 40 + i))
        for k in ("grad", "xgrad"):
            assert np.array_equal(got[k].view(np.uint16), want[k].view(np.uint16)), (i, k)
        sa, sb = got["stats"].copy(), want["stats"].copy()
        l2_diff = np.flatnonzero(sa[:, 3].view(np.uint32) != sb[:, 3].view(np.uint32))
        l2_bits += len(l2_diff)
        if len(l2_diff):
            print("layout %d: l2_term of sequence(s) %s: %s against %s" % (i, l2_diff, sa[l2_diff, 3], sb[l2_diff, 3]))
        sa[:, 3] = sb[:, 3] = 0
        assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), i
        ra, rb = _res_tuple(got["res"]), _res_tuple(want["res"])
        assert ra[:1] + ra[2:] == rb[:1] + rb[2:], (i, ra, rb)       # (index 1: l2_term)
        assert got["xres"] == want["xres"], i
        assert got["res"].num_ok == len(seqs) and got["res"].frames == int(r.frames.sum())
        for k in ("grad", "xgrad"):
            assert np.all(got[k][~r.sup] == cr.SENTINEL) and not np.all(got[k][r.sup] == cr.SENTINEL), (i, k)
        f.close()
        r.close()
        for h in one[::-1]:
            h.close()
    for h in live[::-1]:
        h.close()
    print("l2_term: %d of %d per-sequence statistics differ in their last bits" % (l2_bits, sum(len(s) for s, _ in layouts)))


# ---------------------------------------------------------------------------
# §6 no switch grows the net when it is set again
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SWITCHES) + ["two-seeds"])
def test_switching_again_allocates_nothing(gpu, name):
    """nnet_debug_alloc_count after on / off / on five times equals the count after the first on
    (each with a step, so that what a mode allocates at its first forward or backward is counted)"""
    kf = gpu
    if name == "two-seeds":
        live = Recipe("tiny_xent").make(kf)
        cycle = lambda on: live.step(300, two_seeds=on)
    else:
        cfg, base, sw, seqs = SWITCHES[name]
        live = Recipe(cfg, *base).make(kf)

        def cycle(on):
            live.switch(sw, on)
            live.step(300, seq=SEQS[300] if seqs else None)
    cycle(False)    # (what the step allocates at its first run whatever the switch says, e.g. a conv's transposed taps)
    cycle(True)
    first = live.net.debug_alloc_count()
    assert first > 0
    for _ in range(5):
        cycle(False)
        cycle(True)
    assert live.net.debug_alloc_count() == first, name
    live.close()
