"""Cost of the ReLU unit statistics and self-repair, which bench.py does not switch
on. Reported, not gated:

1. the row-subsampled train step of configs/cnn_tdnn_17f.xconfig (64 egs, chain objective, SGD;
   inputs resident) with training-mode BatchNorm on the sites "all" and "tdnnf", self-repair off and
   on alternating within this one process: median [min .. max] of the timed steps per round (host
   clock around steps that end in a device synchronise).
2. per launch (HIP events around each entry on the library stream, entries interleaved) at the
   compact rows of that model, [tc x 1536] fp16: each new entry beside its existing counterpart on
   the same tensor, and kf_relu_repair_vectors over a table of 17 sites of 1536 columns.

  python scripts/self_repair_bench.py [--egs 64] [--steps 10] [--rounds 3] [--reps 30]
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
net.set_row_subsampling(3)
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
TC = {}


def train_step():
    net.forward(fb.ptr, T)
    objective.compute(nbatch, out_ptr, P, TC["tc"], (row0 // 3).astype(np.int32), nfr, 1, gbuf.ptr, P)
    net.backward(gbuf.ptr)
    net.sgd(1e-8, 0.9)


CONFIGS = [("%s / %s" % (sites, "on" if on else "off"), sites, on) for sites in ("all", "tdnnf") for on in (False, True)]


def timed(sites, on):
    net.set_self_repair(False)
    net.set_batchnorm_train(False)
    net.set_batchnorm_train_sites(sites)
    net.set_batchnorm_train(True)
    net.set_self_repair(on)
    assert bool(net.self_repair_sites()) == on
    net.forward(fb.ptr, T)
    TC["tc"], TC["tc0"], _ = net.row_set()
    assert TC["tc"] > 0
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
    return sorted(ms)


res = {c[0]: [] for c in CONFIGS}
for _ in range(args.rounds):
    for name, sites, on in CONFIGS:
        res[name].append(timed(sites, on))
print("row-subsampled train step, cnn_tdnn_17f, %d egs (T = %d, tc = %d, tc0 = %d), BatchNorm-train sites / self-repair, "
      "ms per step: median [min .. max] of %d, per round" % (args.egs, T, TC["tc"], TC["tc0"], args.steps))
for name, _, _ in CONFIGS:
    allms = sorted(x for m in res[name] for x in m)
    print("  %-12s " % name + "  ".join("%.2f [%.2f .. %.2f]" % (m[len(m) // 2], m[0], m[-1]) for m in res[name])
          + "   | median of the rounds' medians %.2f, all steps %.2f [%.2f .. %.2f]"
          % (sorted(m[len(m) // 2] for m in res[name])[len(res[name]) // 2], allms[len(allms) // 2], allms[0], allms[-1]))
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
dz = kf.DeviceBuffer(tensor)
mask = kf.upload_f32(rng.integers(0, 2 ** 31, size=(tc * D // 32 + 4,), dtype=np.int64).astype(np.int32).view(np.float32))
st = kf.upload_f32(np.zeros(4 * D, np.float32))
ab = kf.upload_f32(np.zeros(2 * D, np.float32))
acc = kf.upload_f32(np.zeros(2 * (2 + 2 * D), np.float32))
NS = 17
racc = kf.upload_f32(np.zeros(NS * 2 * (2 + D), np.float32))
sv = kf.upload_f32((rng.integers(-1, 2, NS * D) * np.float32(1e-5)).astype(np.float32))
tab = (kf.KfRepairSite * NS)(*[kf.KfRepairSite(racc.ptr + 8 * (2 + D) * i, racc.ptr + 8 * (2 + D) * i + 16, sv.ptr + 4 * D * i, D,
                                               1e-5, 0.05, 0.95) for i in range(NS)])
tab_dev = kf.upload_f32(np.frombuffer(bytes(tab), np.float32))
p = lambda k: st.ptr + 4 * D * k  # noqa: E731
A = (acc.ptr, acc.ptr + 16, acc.ptr + 16 + 8 * D)
BW = (g.ptr, D, r.ptr, D, tc)


def f_stats():
    kf.check(kf.core.kf_bn_train_stats(r.ptr, D, tc0, D, 1e-3, 1.0, p(0), p(1), p(2), p(3), *A))


def f_stats_relu():
    kf.check(kf.core.kf_bn_train_stats_relu(r.ptr, D, tc0, D, 1e-3, 1.0, p(0), p(1), p(2), p(3), *A, racc.ptr, racc.ptr + 16))


def f_vectors():
    kf.check(kf.core.kf_relu_repair_vectors(C.byref(tab), tab_dev.ptr, NS, None))


def f_apply():
    kf.check(kf.core.kf_bn_train_bwd_apply(*BW, D, p(2), p(3), 1.0, ab.ptr, ab.ptr + 4 * D, None, 0, None, mask.ptr, D, dz.ptr, D))


def f_apply_repair():
    kf.check(kf.core.kf_bn_train_bwd_apply_repair(*BW, D, p(2), p(3), 1.0, ab.ptr, ab.ptr + 4 * D, None, 0, None, mask.ptr, D,
                                                  dz.ptr, D, sv.ptr))


def f_rows():
    kf.check(kf.core.kf_bn_train_bwd_apply_rows(*BW, tc0, D, p(2), p(3), 1.0, ab.ptr, ab.ptr + 4 * D, None, 0, None, mask.ptr, D,
                                                dz.ptr, D))


def f_rows_repair():
    kf.check(kf.core.kf_bn_train_bwd_apply_rows_repair(*BW, tc0, D, p(2), p(3), 1.0, ab.ptr, ab.ptr + 4 * D, None, 0, None,
                                                       mask.ptr, D, dz.ptr, D, sv.ptr))


rows = [("kf_bn_train_stats (rows = tc0 = %d)" % tc0, f_stats, tc0 * D * 2),
        ("kf_bn_train_stats_relu", f_stats_relu, tc0 * D * 2),
        ("kf_bn_train_bwd_apply (rows = tc = %d)" % tc, f_apply, 3 * tensor + tensor // 16),
        ("kf_bn_train_bwd_apply_repair (both launches)", f_apply_repair, 3 * tensor + tensor // 16 + 4 * D),
        ("kf_bn_train_bwd_apply_rows (tc, tc0)", f_rows, 3 * tensor + tensor // 16),
        ("kf_bn_train_bwd_apply_rows_repair (both launches)", f_rows_repair, 3 * tensor + tensor // 16 + 4 * D),
        ("kf_relu_repair_vectors (%d sites x %d)" % (NS, D), f_vectors, NS * D * 12)]
res = timeit([f for _, f, _ in rows], args.reps)
print("per entry at [%d x %d] (us: median, min, max of %d; events around each entry, every launch of an entry inside)"
      % (tc, D, args.reps))
for (name, _, nbytes), (med, lo, hi) in zip(rows, res):
    print("  %-50s %8.1f %8.1f %8.1f   %6.1f MB -> %5.0f GB/s [%5.0f .. %5.0f]" % (
        name, med, lo, hi, nbytes * 1e-6, nbytes / med * 1e-3, nbytes / hi * 1e-3, nbytes / lo * 1e-3))
