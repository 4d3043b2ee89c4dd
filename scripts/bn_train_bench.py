"""Cost of the TDNN-F training-mode BatchNorm, which bench.py does not switch on.
Reported, not gated:

1. per launch (HIP events around each entry on the library stream) on the benchmark model's
   TDNN-F output, T = egs x 1500 rows of 1536 columns: kf_bn_train_stats, kf_bn_train_apply (with
   bypass; with and without dropout), kf_bn_train_bwd_stats, kf_bn_train_bwd_apply, each beside
   the bytes it must move and the bandwidth that gives, and ops_copy of the same tensor as the HBM
   yardstick of a pass that reads and writes [T x 1536] fp16.
2. the all-rows train step of configs/cnn_tdnn_17f.xconfig (64 egs, chain objective, SGD; inputs
   resident; row subsampling off, which the mode needs) with the switch off and on, alternating:
   median and spread of the timed steps (host clock around steps that end in a device synchronise).

  python scripts/bn_train_bench.py [--egs 64] [--steps 10] [--rounds 3] [--skip-step]
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
FRAMES, D = 1500, 1536
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


# ---- 1. per launch
rng = np.random.default_rng(0)
tensor = T * D * 2                                         # bytes of one [T x D] fp16 tensor
r = kf.upload_fp16(np.maximum(rng.standard_normal((T, D), dtype=np.float32) + 0.3, 0).astype(np.float16))
x = kf.upload_fp16(rng.standard_normal((T, D), dtype=np.float32).astype(np.float16))
g = kf.upload_fp16((rng.standard_normal((T, D), dtype=np.float32) * 0.1).astype(np.float16))
out, dz = kf.DeviceBuffer(tensor), kf.DeviceBuffer(tensor)
mask = kf.DeviceBuffer(T * D // 8)
kf.core.bridge_gpu_memset(mask.ptr, 0xA5, T * D // 8)
st = kf.upload_f32(np.zeros(4 * D, np.float32))
ab = kf.upload_f32(np.zeros(2 * D, np.float32))
acc = kf.upload_f32(np.zeros(2 * (2 + 2 * D), np.float32))
drop = kf.upload_f32(rng.uniform(0.4, 1.6, size=(B, D)).astype(np.float32))
seg = kf.upload_f32(np.repeat(np.arange(B, dtype=np.int32), FRAMES).view(np.float32))
p = lambda k: st.ptr + 4 * D * k  # noqa: E731


def f_stats():
    kf.check(kf.core.kf_bn_train_stats(r.ptr, D, T, D, 1e-3, 1.0, p(0), p(1), p(2), p(3), acc.ptr, acc.ptr + 16,
                                       acc.ptr + 16 + 8 * D))


def f_apply():
    kf.check(kf.core.kf_bn_train_apply(r.ptr, D, T, D, p(2), p(3), None, 0, None, x.ptr, D, 0.66, out.ptr, D))


def f_apply_drop():
    kf.check(kf.core.kf_bn_train_apply(r.ptr, D, T, D, p(2), p(3), drop.ptr, D, seg.ptr, x.ptr, D, 0.66, out.ptr, D))


def f_bstats():
    kf.check(kf.core.kf_bn_train_bwd_stats(g.ptr, D, r.ptr, D, T, D, p(2), p(3), 1.0, None, 0, None, ab.ptr, ab.ptr + 4 * D))


def f_bapply():
    kf.check(kf.core.kf_bn_train_bwd_apply(g.ptr, D, r.ptr, D, T, D, p(2), p(3), 1.0, ab.ptr, ab.ptr + 4 * D, None, 0, None,
                                           mask.ptr, D, dz.ptr, D))


def f_copy():
    kf.check(kf.core.ops_copy(out.ptr, r.ptr, T * D))


rows = [("kf_bn_train_stats", f_stats, tensor), ("kf_bn_train_apply", f_apply, 3 * tensor),
        ("kf_bn_train_apply+drop", f_apply_drop, 3 * tensor), ("kf_bn_train_bwd_stats", f_bstats, 2 * tensor),
        ("kf_bn_train_bwd_apply", f_bapply, 3 * tensor + tensor // 16), ("ops_copy", f_copy, 2 * tensor)]
res = timeit([f for _, f, _ in rows], args.reps)
print("per entry, [%d x %d] fp16 (us: median, min, max of %d; events around each entry, both launches of a statistics "
      "entry inside)" % (T, D, args.reps))
for (name, _, nbytes), (med, lo, hi) in zip(rows, res):
    print("  %-24s %8.1f %8.1f %8.1f   %6.1f MB -> %5.0f GB/s" % (name, med, lo, hi, nbytes * 1e-6, nbytes / med * 1e-3))
if args.skip_step:
    sys.exit(0)
for b in (r, x, g, out, dz, mask, drop, seg):
    b.free()

# ---- 2. the all-rows train step
net = kf.Network(synth.load_xconfig("cnn_tdnn_17f.xconfig"), max_frames=T)
synth.init_network(net, seed=42)
names = [n for n, *_ in net.layers]
P = net.layers[names.index("output")][3]
dgraph = chain.DenGraph(synth.make_den_graph(num_pdfs=P))
nbatch = chain.NumBatch(chain.pack_num_fsts([synth.make_num_fst(e, num_pdfs=P) for e in range(args.egs)]))
row0, nfr, stride = synth.chain_layout(args.egs, FRAMES)
objective = chain.Chain(dgraph, max_seqs=args.egs, max_frames=int(nfr.max()))
fb = kf.upload_fp16(synth.make_features(T, 40))
gbuf = kf.DeviceBuffer(T * P * 2)
kf.core.bridge_gpu_memset(gbuf.ptr, 0, T * P * 2)
out_ptr = net.activation("output")[0]


def train_step():
    net.forward(fb.ptr, T)
    objective.compute(nbatch, out_ptr, P, T, row0, nfr, stride, gbuf.ptr, P)
    net.backward(gbuf.ptr)
    net.sgd(1e-8, 0.9)


def timed(on):
    net.set_batchnorm_train(on)
    for _ in range(2):
        train_step()
    kf.sync()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        train_step()
        kf.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)


res = {False: [], True: []}
for _ in range(args.rounds):
    for on in (False, True):
        res[on].append(timed(on))
print("all-rows train step, cnn_tdnn_17f, %d egs, %d governed layers, ms per step (median [min .. max] of %d, per round):"
      % (args.egs, len(net.batchnorm_train_layers()), args.steps))
for on in (False, True):
    print("  training-mode BatchNorm %-3s " % ("on" if on else "off")
          + "  ".join("%.2f [%.2f .. %.2f]" % (m[len(m) // 2], m[0], m[-1]) for m in res[on]))
r_ = objective.result()
print("last objective / frame %.4f (%d of %d egs ok)" % (r_.objf / max(r_.frames, 1), r_.num_ok, args.egs))
