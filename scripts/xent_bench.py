"""Cost of training the xent branch, which bench.py does not switch on.
Reported, not gated:

1. kf_chain_xent alone (HIP events around each call on the library stream) at the benchmark's
   shape: 64 egs of 490 supervised frames, P pdfs, the compact stride-1 layout, after one real
   kf_chain_compute; beside it, in the same call, ops_copy of as many bytes (the kernel reads
   the fp16 log-softmax rows and writes the fp16 gradient rows: 4 P bytes per row) as the HBM
   yardstick.
2. the row-subsampled train step of configs/cnn_tdnn_17f_kaldi.xconfig (64 egs, ivector front
   end, chain objective, SGD; inputs resident) without and with the xent output trained
   (Chain.xent + the backward with two seeds), alternating: median and spread of the timed steps
   (host clock around steps that end in a device synchronise).

  python scripts/xent_bench.py [--egs 64] [--steps 10] [--rounds 3] [--skip-step]
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
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--skip-step", action="store_true")
args = ap.parse_args()

kf.check(kf.core.bridge_gpu_init(0))
FRAMES = 1500
T, B = args.egs * FRAMES, args.egs

# the HIP runtime the library runs on (the one mapped copy): events with timing
hip = C.CDLL(kf.hip_runtimes()[0])
for name, argt in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                   ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
    getattr(hip, name).argtypes, getattr(hip, name).restype = argt, C.c_int


def event():
    e = C.c_void_p()
    assert hip.hipEventCreate(C.byref(e)) == 0
    return e


def timeit(fns, reps):
    """us per call of each fn: HIP events around every call, the fns interleaved (median, min, max)"""
    stream = kf.core.kf_get_stream()
    for fn in fns:
        for _ in range(3):
            fn()
    kf.sync()
    ev = [[(event(), event()) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for i, fn in enumerate(fns):
            a, b = ev[i][r]
            assert hip.hipEventRecord(a, stream) == 0
            fn()
            assert hip.hipEventRecord(b, stream) == 0
    kf.sync()
    out = []
    for i in range(len(fns)):
        us = []
        for a, b in ev[i]:
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
            us.append(1e3 * ms.value)
        us.sort()
        out.append((us[len(us) // 2], us[0], us[-1]))
    return out


# ---- the model, its forward on the row set and the objective's compact layout (as bench.py)
xcfg = synth.load_xconfig("cnn_tdnn_17f_kaldi.xconfig")
net = kf.Network(xcfg, max_frames=T)
synth.init_network(net, seed=42)
net.set_row_subsampling(3)
names = [n for n, *_ in net.layers]
P = net.layers[names.index("output")][3]
assert net.layers[names.index("output-xent")][3] == P
dgraph = chain.DenGraph(synth.make_den_graph(num_pdfs=P))
nbatch = chain.NumBatch(chain.pack_num_fsts([synth.make_num_fst(e, num_pdfs=P) for e in range(B)]))
row0, nfr, stride = synth.chain_layout(B, FRAMES)
objective = chain.Chain(dgraph, max_seqs=B, max_frames=int(nfr.max()))
fb = kf.upload_fp16(synth.make_features(T, 40))
iv = kf.upload_fp16((np.random.default_rng(99).standard_normal((B, 100)) * 2).astype(np.float16))
seq_off = np.arange(B + 1, dtype=np.int32) * FRAMES
net.forward_ivector(fb.ptr, T, iv.ptr, seq_off)
tc, tc0, _ = net.row_set()
assert tc and stride == 3 and np.all(row0 % 3 == 0), "the row set was not used"
rows, crow0 = tc, row0 // 3
gbuf, xbuf = kf.DeviceBuffer(rows * P * 2), kf.DeviceBuffer(rows * P * 2)
kf.core.bridge_gpu_memset(gbuf.ptr, 0, rows * P * 2)
kf.core.bridge_gpu_memset(xbuf.ptr, 0, rows * P * 2)
out_ptr, xent_ptr = net.activation("output")[0], net.activation("output-xent")[0]
o = chain.KfChainOpts.default()
opts = chain.KfChainOpts(o.l2_regularize, o.out_of_range_regularize, o.leaky_hmm_coefficient, 0.1, o.supervision_weight)

# ---- 1. the kernel alone
objective.compute(nbatch, out_ptr, P, rows, crow0, nfr, 1, gbuf.ptr, P, opts)
nbytes = int(nfr.sum()) * 4 * P
src, dst = kf.DeviceBuffer(nbytes // 2), kf.DeviceBuffer(nbytes // 2)
kf.core.bridge_gpu_memset(src.ptr, 0, nbytes // 2)


def f_xent():
    objective.xent(nbatch, xent_ptr, P, xbuf.ptr, P, opts)


def f_copy():
    kf.check(kf.core.ops_copy(dst.ptr, src.ptr, nbytes // 4))


res = timeit([f_xent, f_copy], args.reps)
print("%d egs x %d frames, P = %d (us: median, min, max of %d; events around each call)" % (B, int(nfr.max()), P, args.reps))
for name, (med, lo, hi) in zip(("kf_chain_xent", "ops_copy"), res):
    print("  %-16s %8.1f %8.1f %8.1f   %6.1f MB -> %5.0f GB/s" % (name, med, lo, hi, nbytes * 1e-6, nbytes / med * 1e-3))
xo, xw = objective.xent_result()
print("xent objective / frame %.4f (-log P = %.4f)" % (xo / xw, -np.log(P)))
if args.skip_step:
    sys.exit(0)
src.free()
dst.free()


# ---- 2. the train step
def train_step(xent):
    net.forward_ivector(fb.ptr, T, iv.ptr, seq_off)
    objective.compute(nbatch, out_ptr, P, rows, crow0, nfr, 1, gbuf.ptr, P, opts)
    if xent:
        objective.xent(nbatch, xent_ptr, P, xbuf.ptr, P, opts)
        net.backward(gbuf.ptr, xbuf.ptr)
    else:
        net.backward(gbuf.ptr)
    net.sgd(1e-8, 0.9)


def timed(xent):
    for _ in range(2):
        train_step(xent)
    kf.sync()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        train_step(xent)
        kf.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)


res = {False: [], True: []}
for _ in range(args.rounds):
    for xent in (False, True):
        res[xent].append(timed(xent))
print("row-subsampled train step, cnn_tdnn_17f_kaldi, %d egs, ms per step (median [min .. max] of %d, per round):"
      % (B, args.steps))
for xent in (False, True):
    print("  xent output %-11s " % ("trained" if xent else "not trained")
          + "  ".join("%.2f [%.2f .. %.2f]" % (m[len(m) // 2], m[0], m[-1]) for m in res[xent]))
r_ = objective.result()
print("last objective / frame %.4f (%d of %d egs ok)" % (r_.objf / max(r_.frames, 1), r_.num_ok, B))
