"""Cost of the dynamic loss scale, which bench.py does not switch on. Reported,
not gated:

1. the train step of configs/cnn_tdnn_17f.xconfig (64 egs, chain objective; inputs resident), row
   subsampled as bench.py's headline step, with the loss scale off and on, alternating within this
   one process, several rounds, for both parameter steps:
     sgd    / off, on      Network.sgd
     update / off, on      Network.update (the Kaldi-style update)
   median [min .. max] of the timed steps per round (host clock around steps that end in a device
   synchronise). On: one more read of the gradient buffer (the check pass) and two small launches.
2. per launch (HIP events around each entry on the library stream, entries interleaved) over the
   model's flat parameter set: kf_loss_scale_check (both launches), the plain and the scaled
   update entries, each beside the bytes it has to move.

  python scripts/loss_scale_bench.py [--egs 64] [--steps 10] [--rounds 3] [--reps 30]
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
FRAMES = 1500
T = args.egs * FRAMES

# ---- 1. the train step
net = kf.Network(synth.load_xconfig("cnn_tdnn_17f.xconfig"), max_frames=T)
synth.init_network(net, seed=42)
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
net.set_row_subsampling(3)
net.forward(fb.ptr, T)
tc, _tc0, _ = net.row_set()
assert tc > 0
crow0 = (row0 // 3).astype(np.int32)
kf.core.bridge_gpu_memset(gbuf.ptr, 0, T * P * 2)


def train_step(update):
    net.forward(fb.ptr, T)
    objective.compute(nbatch, out_ptr, P, tc, crow0, nfr, 1, gbuf.ptr, P)
    net.backward(gbuf.ptr)
    if update:
        net.update(1e-8, 0.9, 2.0, float(nfr.sum()))
    else:
        net.sgd(1e-8, 0.9)


CONFIGS = [("sgd / off", False, False), ("sgd / on", False, True), ("update / off", True, False),
           ("update / on", True, True)]
SKIPS = {}


def timed(name, update, on):
    net.set_loss_scale(on, growth_interval=1 << 30)   # (init_scale 65536, the reference's training scale)
    objective.set_grad_scale(net.loss_scale_ptr() if on else None)
    for _ in range(2):
        train_step(update)
    kf.sync()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        train_step(update)
        kf.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    r = objective.result()
    assert r.num_ok == args.egs and np.isfinite(r.objf)
    if on:
        st = net.loss_scale_stats()
        SKIPS[name] = (st["skipped"], st["steps"], st["scale"])
    return sorted(ms), r.objf / max(r.frames, 1)


res = {c[0]: [] for c in CONFIGS}
objf = {}
for _ in range(args.rounds):
    for name, update, on in CONFIGS:
        ms, objf[name] = timed(name, update, on)
        res[name].append(ms)
print("train step, cnn_tdnn_17f, %d egs (T = %d, compact rows tc = %d), %d parameters, ms per step: median [min .. max] of %d, per round"
      % (args.egs, T, tc, net.num_params, args.steps))
for name, _, _ in CONFIGS:
    allms = sorted(x for m in res[name] for x in m)
    print("  %-13s " % name + "  ".join("%.2f [%.2f .. %.2f]" % (m[len(m) // 2], m[0], m[-1]) for m in res[name])
          + "   | all rounds %.2f [%.2f .. %.2f], objective / frame %.4f" % (allms[len(allms) // 2], allms[0], allms[-1], objf[name])
          + ("" if name not in SKIPS else ", last round: %d of %d steps skipped, scale %g" % SKIPS[name]))
n = net.num_params
net.set_loss_scale(False)
objective.set_grad_scale(None)
net.close()
for b in (fb, gbuf):
    b.free()

# ---- 2. per launch over a flat parameter set of the model's size
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


# eight components of one segment each, with 64 elements of padding between them
rng = np.random.default_rng(0)
ncomp = 8
per = (n // ncomp) // 64 * 64 - 64
seg_rows, comp_rows, wg = [], [], 0
for c in range(ncomp):
    b = c * (per + 64)
    nwg = -(-per // kf.UPD_CHUNK)
    seg_rows.append(kf.KfUpdSegment(b, b + per, c, wg))
    comp_rows.append(kf.KfUpdComp(0.75, 0.0, 1.0, wg, nwg))
    wg += nwg
sa, ca = (kf.KfUpdSegment * ncomp)(*seg_rows), (kf.KfUpdComp * ncomp)(*comp_rows)
segs, comps = kf.DeviceBuffer(C.sizeof(sa)), kf.DeviceBuffer(C.sizeof(ca))
kf.check(kf.core.bridge_transfer_int32(segs.ptr, C.addressof(sa), C.sizeof(sa) // 4))
kf.check(kf.core.bridge_transfer_int32(comps.ptr, C.addressof(ca), C.sizeof(ca) // 4))
w = kf.upload_f32((rng.standard_normal(n, dtype=np.float32) * 0.1))
g = kf.upload_f32(rng.standard_normal(n, dtype=np.float32))
v = kf.upload_f32(np.zeros(n, np.float32))
h = kf.DeviceBuffer(n * 2)
scratch = kf.DeviceBuffer(kf.core.kf_update_scratch_bytes(n, ncomp, ncomp))
stats = kf.DeviceBuffer((2 * ncomp + 2) * 4)
state = kf.DeviceBuffer(kf.core.kf_loss_scale_state_bytes())
flags = kf.DeviceBuffer(kf.core.kf_loss_scale_scratch_bytes(n, ncomp))
o = kf.KfLossScaleOpts()
kf.core.kf_loss_scale_default_opts(C.byref(o))
o.init_scale, o.growth_interval = 1.0, 1 << 30
kf.check(kf.core.kf_loss_scale_init(state.ptr, C.byref(o)))
upd = (w.ptr, h.ptr, g.ptr, v.ptr, n, segs.ptr, ncomp, comps.ptr, ncomp, 1e-8, 0.9, 2.0, 1.0, scratch.ptr, stats.ptr)


def f_check():
    kf.check(kf.core.kf_loss_scale_check(state.ptr, g.ptr, n, segs.ptr, ncomp, ncomp, flags.ptr))


def f_update():
    kf.check(kf.core.kf_update_maxchange(*upd))


def f_update_scaled():
    kf.check(kf.core.kf_update_maxchange_scaled(*upd, state.ptr))


def f_sgd():
    kf.check(kf.core.kf_sgd_flat(w.ptr, h.ptr, g.ptr, v.ptr, 1e-8, 0.9, n))


def f_sgd_scaled():
    kf.check(kf.core.kf_sgd_flat_scaled(w.ptr, h.ptr, g.ptr, v.ptr, 1e-8, 0.9, n, state.ptr))


cov = ncomp * per
rows = [("kf_loss_scale_check (check + advance)", f_check, 4 * cov),
        ("kf_update_maxchange", f_update, 26 * cov),
        ("kf_update_maxchange_scaled", f_update_scaled, 26 * cov),
        ("kf_sgd_flat", f_sgd, 22 * n),
        ("kf_sgd_flat_scaled", f_sgd_scaled, 22 * n)]
res = timeit([f for _, f, _ in rows], args.reps)
print("per entry over %d parameters (us: median, min, max of %d; events around each entry, every launch of it inside)" % (n, args.reps))
for (name, _, nbytes), (med, lo, hi) in zip(rows, res):
    print("  %-40s %8.1f %8.1f %8.1f   %6.1f MB -> %5.0f GB/s [%5.0f .. %5.0f]" % (
        name, med, lo, hi, nbytes * 1e-6, nbytes / med * 1e-3, nbytes / hi * 1e-3, nbytes / lo * 1e-3))
