"""Cost of the egs' weights inside the chain objective, which bench.py does not
switch on. Reported, not gated.

The objective at the benchmark's shape: 64 egs of 490 supervised frames, P = 3080 pdfs, the
compact stride-1 layout, random fp16 outputs (the objective's time does not depend on their
values), compute followed by kf_chain_xent. Three variants alternate call by call in one
process: no weights (kf_chain_compute), a ramp of deriv weights with per-eg weights
(kf_chain_compute_weighted), and all weights 1.0 through the weighted entry. Per variant: the
device time between HIP events around compute + xent on the library stream with the calls queued
back to back, and, in a second pass on an idle device, the host time the two calls take to
return (the weighted entry validates and stages B x frames floats).
Median of each round, then the median and the spread of the rounds' medians.

  python scripts/deriv_weights_bench.py [--egs 64] [--reps 20] [--rounds 5]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kaldi-fp16_amd", "python"))
import numpy as np  # noqa: E402
import kfp16 as kf  # noqa: E402
from kfp16 import chain, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--egs", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

kf.check(kf.core.bridge_gpu_init(0))
B, FRAMES, P = args.egs, 1500, 3080

hip = C.CDLL(kf.hip_runtimes()[0])
for name, argt in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                   ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
    getattr(hip, name).argtypes, getattr(hip, name).restype = argt, C.c_int


def event():
    e = C.c_void_p()
    assert hip.hipEventCreate(C.byref(e)) == 0
    return e


dgraph = chain.DenGraph(synth.make_den_graph(num_pdfs=P))
nbatch = chain.NumBatch(chain.pack_num_fsts([synth.make_num_fst(e, num_pdfs=P) for e in range(B)]))
row0, nfr, stride = synth.chain_layout(B, FRAMES)
crow0 = (np.arange(B) * int(nfr.max())).astype(np.int32)       # compact rows, stride 1
rows = int(nfr.sum())
objective = chain.Chain(dgraph, max_seqs=B, max_frames=int(nfr.max()))
rng = np.random.default_rng(3)
x = kf.upload_fp16((rng.standard_normal((rows, P)) * 2).astype(np.float16))
y = (rng.standard_normal((rows, P)) * 2).astype(np.float32)
y -= np.log(np.exp(y).sum(1, keepdims=True))
y = kf.upload_fp16(y.astype(np.float16))
gbuf, xbuf = kf.DeviceBuffer(rows * P * 2), kf.DeviceBuffer(rows * P * 2)
o = chain.KfChainOpts.default()
opts = chain.KfChainOpts(5e-5, o.out_of_range_regularize, o.leaky_hmm_coefficient, 0.1, o.supervision_weight)

ramp = np.concatenate([np.linspace(0.1, 1.0, int(n)) for n in nfr]).astype(np.float32)
egw = rng.uniform(0.5, 2.0, B).astype(np.float32)
VARIANTS = (("no weights", None, None), ("weighted", egw, ramp),
            ("all ones", np.ones(B, np.float32), np.ones(rows, np.float32)))


def call(sw, fw):
    objective.compute(nbatch, x.ptr, P, rows, crow0, nfr, 1, gbuf.ptr, P, opts, seq_weight=sw, frame_weight=fw)
    objective.xent(nbatch, y.ptr, P, xbuf.ptr, P, opts)


stream = kf.core.kf_get_stream()
for _, sw, fw in VARIANTS:
    for _ in range(3):
        call(sw, fw)
kf.sync()
dev = {n: [] for n, *_ in VARIANTS}
host = {n: [] for n, *_ in VARIANTS}
for _ in range(args.rounds):
    ev = {n: [(event(), event()) for _ in range(args.reps)] for n, *_ in VARIANTS}
    hs = {n: [] for n, *_ in VARIANTS}
    # device time: the calls queued back to back (the host runs ahead of the device, so the
    # events bracket device work alone)
    for r in range(args.reps):
        for n, sw, fw in VARIANTS:
            a, b = ev[n][r]
            assert hip.hipEventRecord(a, stream) == 0
            call(sw, fw)
            assert hip.hipEventRecord(b, stream) == 0
    kf.sync()
    # host time: each call on an idle device, so no wait for a staging slot or a full queue is in it
    for r in range(args.reps):
        for n, sw, fw in VARIANTS:
            t0 = time.perf_counter()
            call(sw, fw)
            hs[n].append((time.perf_counter() - t0) * 1e6)
            kf.sync()
    for n, *_ in VARIANTS:
        us = []
        for a, b in ev[n]:
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
            us.append(1e3 * ms.value)
        dev[n].append(float(np.median(us)))
        host[n].append(float(np.median(hs[n])))

print("%d egs x %d frames, P = %d, compute + xent; us, median [min .. max] of %d rounds' medians (%d calls each)"
      % (B, int(nfr.max()), P, args.rounds, args.reps))
for n, *_ in VARIANTS:
    d, h = dev[n], host[n]
    print("  %-11s device %8.1f [%8.1f .. %8.1f]   host enqueue %7.1f [%7.1f .. %7.1f]"
          % (n, np.median(d), min(d), max(d), np.median(h), min(h), max(h)))
r_ = objective.result()
print("last objective / frame %.4f (%d of %d egs ok)" % (r_.objf / max(r_.frames, 1), r_.num_ok, B))
