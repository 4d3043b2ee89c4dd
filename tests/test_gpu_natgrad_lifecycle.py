"""A net that used natural-gradient preconditioning, closed and opened again in one process,
leaves no pending HIP error (the pattern of tests/test_gpu_lifecycle.py)."""
import numpy as np
import pytest


@pytest.mark.gpu
def test_close_and_reopen_after_natural_gradient(gpu):
    kf = gpu
    from kfp16 import synth
    kf.core.kf_pending_clear()
    T = 150
    xcfg = synth.load_xconfig("tiny.xconfig")
    feats = kf.upload_fp16(synth.make_features(T, 40, seed=2))
    grads = []
    for _ in range(2):
        net = kf.Network(xcfg, max_frames=T)
        synth.init_network(net, seed=3)
        net.set_natural_gradient(True)
        net.forward(feats.ptr, T)
        out = net.read_activation("output")
        og = kf.upload_fp16((np.random.default_rng(2).standard_normal(out.shape) * 0.05).astype(np.float16))
        for _ in range(2):
            net.backward(og.ptr)
        net.sgd(1e-4, 0.9)
        assert not any(r["flag"] for r in net.natural_gradient_stats())
        grads.append(kf.read_f32(net.grad_ptr, (net.num_params,)))
        net.close()
        kf.sync()
        assert kf.core.kf_peek_error() == 0
        assert kf.pending_log() is None, kf.pending_log()
    # the second life starts from the default initial state: the same bits
    assert np.array_equal(grads[0].view(np.uint32), grads[1].view(np.uint32))
