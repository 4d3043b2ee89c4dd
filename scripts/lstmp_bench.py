"""The projected LSTM operator at the TDNN-LSTM recipe's shape, which bench.py does not
run. Reported, not gated: nothing exists to compare it against.

D = 1536, C = 1024, R = N = 256, delay -3, 64 sequences of 160 .. 180 frames (about 170), random
fp16 inputs and parameters. A call is timed twice: by the library's timed-launch records (kf_prof
classes KF_PROF_LSTMP_FWD / _BWD, device events around the whole call on its stream) and by the host
clock from the call to the device synchronise. The median of each round, then the median and the
spread of the rounds' medians, and the launches per call.

  python scripts/lstmp_bench.py [--seqs 64] [--frames 170] [--reps 5] [--rounds 3]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kaldi-fp16_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (the HIP runtime first: the libraries then bind the same copy)
import kfp16 as kf  # noqa: E402
from kfp16 import lstm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seqs", type=int, default=64)
ap.add_argument("--frames", type=int, default=170)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
kf.check(kf.core.bridge_gpu_init(0))
D, C, R, N, DELAY = 1536, 1024, 256, 256, -3
FWD, BWD = 8, 9   # kf_lstm.h KF_PROF_LSTMP_FWD / _BWD

rng = np.random.default_rng(1)
lens = rng.integers(args.frames - 10, args.frames + 11, args.seqs)
seq_row0 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
T = int(seq_row0[-1])
op = lstm.Lstmp(D, C, R, N, DELAY, max_rows=T, max_seqs=args.seqs)
scale = {"W_x": 0.5 / np.sqrt(D), "W_r": 0.5 / np.sqrt(R), "W_p": 1.0 / np.sqrt(C), "b": 0.1, "b_p": 0.1}
op.set_params({k: (rng.standard_normal(s) * scale.get(k, 0.3)).astype(np.float32) for k, s in op.shapes.items()})
x = kf.upload_fp16(rng.standard_normal((T, D)).astype(np.float16))
dy = kf.upload_fp16((rng.standard_normal((T, R + N)) * 0.1).astype(np.float16))
y, dx = kf.DeviceBuffer(T * (R + N) * 2), kf.DeviceBuffer(T * D * 2)
grad = kf.upload_f32(np.zeros(op.num_params))


def fwd():
    op.forward(x.ptr, D, seq_row0, y.ptr, R + N)


def bwd():
    op.backward(dy.ptr, R + N, dx.ptr, D, grad.ptr)


def timed(fn, cls):
    kf.sync()
    kf.core.kf_prof_reset()
    t0 = time.perf_counter()
    fn()
    kf.sync()
    host = (time.perf_counter() - t0) * 1e3
    return host, kf.prof_collect(cls)[1]


for _ in range(2):   # every shape of the timed window, the weight gradients' workspace
    fwd()
    bwd()
kf.sync()

# the forward at this shape against float64 (the tests run small shapes only), batched over sequences
p = {k: v.astype(np.float16).astype(np.float64) for k, v in op.get_params().items()}
xs = kf.read_fp16(x.ptr, (T, D)).astype(np.float64)
sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
y_ref, c_ref = np.zeros((T, R + N)), np.zeros((T, C))
for t in range(int(lens.max())):
    rows = seq_row0[:-1][lens > t] + t
    prev = t + DELAY >= 0
    rp = y_ref[rows + DELAY, :R] if prev else np.zeros((len(rows), R))
    cp = c_ref[rows + DELAY] if prev else np.zeros((len(rows), C))
    ai, af, ag, ao = np.split(xs[rows] @ p["W_x"] + rp @ p["W_r"] + p["b"], 4, axis=1)
    c_ref[rows] = sig(af + p["w_fc"] * cp) * cp + sig(ai + p["w_ic"] * cp) * np.tanh(ag)
    y_ref[rows] = (sig(ao + p["w_oc"] * c_ref[rows]) * np.tanh(c_ref[rows])) @ p["W_p"] + p["b_p"]
y_err = np.linalg.norm(kf.read_fp16(y.ptr, (T, R + N)) - y_ref) / np.linalg.norm(y_ref)
c_err = np.linalg.norm(op.state()["c"] - c_ref) / np.linalg.norm(c_ref)
print("forward against float64 at this shape: y rel err %.2e, c rel err %.2e" % (y_err, c_err))

kf.core.kf_prof_reserve(8)
kf.core.kf_prof_enable(1)
res = {}
for name, fn, cls in (("forward", fwd, FWD), ("backward", bwd, BWD)):
    meds = []
    for _ in range(args.rounds):
        ts = [timed(fn, cls) for _ in range(args.reps)]
        meds.append(np.median(np.array(ts), axis=0))
    meds = np.array(meds)
    res[name] = (np.median(meds, axis=0), meds.max(axis=0) - meds.min(axis=0))
kf.core.kf_prof_enable(0)
steps = -(-int(lens.max()) // -DELAY)
print("lstmp D=%d C=%d R=%d N=%d delay=%d, %d sequences, %d rows, %d steps" % (D, C, R, N, DELAY, args.seqs, T, steps))
print("  launches per call: forward %d (+ the input GEMM), backward %d (+ 4 GEMMs)" % (1 + 2 * steps, 3 * steps - 1 + 2))
for name, (med, spread) in res.items():
    print("  %-8s host clock %8.3f ms (spread of round medians %.3f), device events %8.3f ms (spread %.3f)"
          % (name, med[0], spread[0], med[1], spread[1]))
