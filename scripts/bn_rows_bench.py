"""Cost of the training-mode BatchNorm on the row-subsampled step, which bench.py
does not switch on. Reported, not gated:

1. the train step of configs/cnn_tdnn_17f.xconfig (64 egs, chain objective, SGD; inputs resident)
   in four configurations that alternate within this one process, several rounds:
     rsub / off        the row-subsampled step, frozen BatchNorm (bench.py's headline step)
     rsub / tdnnf      the mode on for the tdnn-f layers, statistics over the rows 0 (mod 3)
     rsub / all        the mode on for every site (the conv below the row set then runs on full
                       rows and is gathered)
     all rows / tdnnf  the all-rows step with the mode on (what §23 measured)
   median [min .. max] of the timed steps per round (host clock around steps that end in a device
   synchronise).
2. per launch (HIP events around each entry on the library stream, entries interleaved) at the
   compact rows of that model, [tc x 1536] fp16: kf_bn_train_stats over tc0 rows, kf_bn_train_apply
   over tc (with the bypass), kf_bn_train_bwd_stats_rows and kf_bn_train_bwd_apply_rows with
   stat_rows = tc0, each beside the bytes it has to move; kf_bn_train_bwd_apply on the same rows
   and ops_copy of the same tensor as yardsticks.

  python scripts/bn_rows_bench.py [--egs 64] [--steps 10] [--rounds 3] [--reps 30]
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
args = ap.parse_args()

kf.check(kf.core.bridge_gpu_init(0))
FRAMES, D = 1500, 1536
T = args.egs * FRAMES

# ---- 1. the train step
net = kf.Network(synth.load_xconfig("cnn_tdnn_17f.xconfig"), max_frames=T)
synth.init_network(net, seed=42)
net.set_batchnorm_train_rows("subsampled")
names = [n for n, *_ in net.layers]
P = net.layers[names.index("output")][3]
dgraph = chain.DenGraph(synth.make_den_graph(num_pdfs=P))
nbatch = chain.NumBatch(chain.pack_num_fsts([synth.make_num_fst(e, num_pdfs=P) for e in range(args.egs)]))
row0, nfr, stride = synth.chain_layout(args.egs, FRAMES)
assert stride == 3 and np.all(row0 % 3 == 0)
objective = chain.Chain(dgraph, max_seqs=args.egs, max_frames=int(nfr.max()))
fb = kf.upload_fp16(synth.make_features(T, 40))
gbuf = kf.DeviceBuffer(T * P * 2)
out_ptr = net.activation("output")[0]
layout = {}                                   # the objective's (rows, row0, stride) of the current configuration


def train_step():
    net.forward(fb.ptr, T)
    rows, r0, st = layout["obj"]
    objective.compute(nbatch, out_ptr, P, rows, r0, nfr, st, gbuf.ptr, P)
    net.backward(gbuf.ptr)
    net.sgd(1e-8, 0.9)


CONFIGS = [("rsub / off", True, None), ("rsub / tdnnf", True, "tdnnf"), ("rsub / all", True, "all"),
           ("all rows / tdnnf", False, "tdnnf")]
TC = {}


def timed(rsub, sites):
    net.set_batchnorm_train(False)
    net.set_row_subsampling(3 if rsub else 0)
    if sites:
        net.set_batchnorm_train_sites(sites)
        net.set_batchnorm_train(True)
    net.forward(fb.ptr, T)                    # the row set of this configuration
    tc, tc0, _ = net.row_set()
    assert (tc > 0) == rsub
    if rsub:
        TC["tc"], TC["tc0"] = tc, tc0
    layout["obj"] = (tc, (row0 // 3).astype(np.int32), 1) if rsub else (T, row0, stride)
    kf.core.bridge_gpu_memset(gbuf.ptr, 0, T * P * 2)
    for _ in range(2):
        train_step()
    kf.sync()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        train_step()
        kf.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    r = objective.result()
    assert r.num_ok == args.egs and np.isfinite(r.objf)
    return sorted(ms), r.objf / max(r.frames, 1)


res = {c[0]: [] for c in CONFIGS}
objf = {}
for _ in range(args.rounds):
    for name, rsub, sites in CONFIGS:
        ms, objf[name] = timed(rsub, sites)
        res[name].append(ms)
print("train step, cnn_tdnn_17f, %d egs (T = %d, compact rows tc = %d, tc0 = %d), ms per step: median [min .. max] of %d, per round"
      % (args.egs, T, TC["tc"], TC["tc0"], args.steps))
for name, _, _ in CONFIGS:
    allms = sorted(x for m in res[name] for x in m)
    print("  %-17s " % name + "  ".join("%.2f [%.2f .. %.2f]" % (m[len(m) // 2], m[0], m[-1]) for m in res[name])
          + "   | all rounds %.2f [%.2f .. %.2f], objective / frame %.4f" % (allms[len(allms) // 2], allms[0], allms[-1], objf[name]))
tc, tc0 = TC["tc"], TC["tc0"]
net.close()
for b in (fb, gbuf):
    b.free()

# ---- 2. per launch at the compact rows
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


rng = np.random.default_rng(0)
tensor = tc * D * 2
r = kf.upload_fp16(np.maximum(rng.standard_normal((tc, D), dtype=np.float32) + 0.3, 0).astype(np.float16))
g = kf.upload_fp16((rng.standard_normal((tc, D), dtype=np.float32) * 0.1).astype(np.float16))
x = kf.upload_fp16(rng.standard_normal((tc, D), dtype=np.float32).astype(np.float16))
out, dz = kf.DeviceBuffer(tensor), kf.DeviceBuffer(tensor)
mask = kf.upload_f32(rng.integers(0, 2 ** 31, size=(tc * D // 32 + 4,), dtype=np.int64).astype(np.int32).view(np.float32))
st = kf.upload_f32(np.zeros(4 * D, np.float32))
ab = kf.upload_f32(np.zeros(2 * D, np.float32))
acc = kf.upload_f32(np.zeros(2 * (2 + 2 * D), np.float32))
p = lambda k: st.ptr + 4 * D * k  # noqa: E731


def f_stats():
    kf.check(kf.core.kf_bn_train_stats(r.ptr, D, tc0, D, 1e-3, 1.0, p(0), p(1), p(2), p(3), acc.ptr, acc.ptr + 16, acc.ptr + 16 + 8 * D))


def f_apply():
    kf.check(kf.core.kf_bn_train_apply(r.ptr, D, tc, D, p(2), p(3), None, 0, None, x.ptr, D, 0.66, out.ptr, D))


def f_bstats():
    kf.check(kf.core.kf_bn_train_bwd_stats_rows(g.ptr, D, r.ptr, D, tc, tc0, D, p(2), p(3), 1.0, None, 0, None, ab.ptr, ab.ptr + 4 * D))


def f_bapply():
    kf.check(kf.core.kf_bn_train_bwd_apply_rows(g.ptr, D, r.ptr, D, tc, tc0, D, p(2), p(3), 1.0, ab.ptr, ab.ptr + 4 * D, None, 0,
                                                None, mask.ptr, D, dz.ptr, D))


def f_bapply_all():
    kf.check(kf.core.kf_bn_train_bwd_apply(g.ptr, D, r.ptr, D, tc, D, p(2), p(3), 1.0, ab.ptr, ab.ptr + 4 * D, None, 0, None,
                                           mask.ptr, D, dz.ptr, D))


def f_copy():
    kf.check(kf.core.ops_copy(out.ptr, r.ptr, tc * D))


rows = [("kf_bn_train_stats (rows = tc0 = %d)" % tc0, f_stats, tc0 * D * 2),
        ("kf_bn_train_apply (rows = tc = %d, bypass)" % tc, f_apply, 3 * tensor),
        ("kf_bn_train_bwd_stats_rows (tc, tc0)", f_bstats, 2 * tensor),
        ("kf_bn_train_bwd_apply_rows (tc, tc0)", f_bapply, 3 * tensor + tensor // 16),
        ("kf_bn_train_bwd_apply (all-rows rule, yardstick)", f_bapply_all, 3 * tensor + tensor // 16),
        ("ops_copy %dx%d (yardstick)" % (tc, D), f_copy, 2 * tensor)]
res = timeit([f for _, f, _ in rows], args.reps)
print("per entry at [%d x %d] (us: median, min, max of %d; events around each entry, both launches of a statistics entry inside)"
      % (tc, D, args.reps))
for (name, _, nbytes), (med, lo, hi) in zip(rows, res):
    print("  %-46s %8.1f %8.1f %8.1f   %6.1f MB -> %5.0f GB/s [%5.0f .. %5.0f]" % (
        name, med, lo, hi, nbytes * 1e-6, nbytes / med * 1e-3, nbytes / hi * 1e-3, nbytes / lo * 1e-3))
