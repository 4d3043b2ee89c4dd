"""Cost of the parameter-side natural gradient of the conv components, which
bench.py does not switch on. Reported, not gated:

1. nnet_backward of configs/cnn_tdnn_17f.xconfig at 64 x 1500 frames (all rows, two streams) with
   natural gradient on, the conv opt-in off and on alternating within this one process: host clock
   around backwards that end in a device synchronise, updating steps (t < 10 or t % 4 == 0) and
   non-updating steps separately, median [min .. max] per round.
2. per launch (HIP events around each entry on the library stream, entries interleaved) on the table
   of that model's six conv components: kf_ng_conv_stats on a non-updating and on an updating step,
   kf_ng_scales, kf_ng_conv_apply and kf_ng_state (updating) on the conv preconditioners.

  python scripts/natgrad_conv_bench.py [--egs 64] [--steps 26] [--rounds 3] [--reps 30]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kaldi-fp16_amd", "python"))
import numpy as np  # noqa: E402
import kfp16 as kf  # noqa: E402
from kfp16 import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--egs", type=int, default=64)
ap.add_argument("--steps", type=int, default=26)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()

kf.check(kf.core.bridge_gpu_init(0))
T = args.egs * 1500

# ---- 1. the backward
net = kf.Network(synth.load_xconfig("cnn_tdnn_17f.xconfig"), max_frames=T)
synth.init_network(net, seed=42)
fb = kf.upload_fp16(synth.make_features(T, 40))
net.forward(fb.ptr, T)
P = net.layers[[n for n, *_ in net.layers].index("output")][3]
rng = np.random.default_rng(0)
og = kf.upload_fp16((rng.standard_normal((T, P), dtype=np.float32) * 0.05).astype(np.float16))
# (K, N) of the conv components, for part 2
convs = [net.params[[t for t in c["tensors"] if net.params[t][0] > 1][0]][:2] for c in net.components()
         if c["name"].startswith("cnn")]


def timed(conv):
    """ms of every backward from the initial state: ([updating], [non-updating])"""
    net.set_natural_gradient(True, conv=conv)
    upd, non = [], []
    for t in range(args.steps):
        kf.sync()
        t0 = time.perf_counter()
        net.backward(og.ptr)
        kf.sync()
        (upd if t < 10 or t % 4 == 0 else non).append((time.perf_counter() - t0) * 1e3)
    rep = net.natural_gradient_stats()
    assert not any(r["flag"] for r in rep) and any(r["name"].startswith("cnn") for r in rep) == conv
    return sorted(upd[2:]), sorted(non)  # (the first two steps warm the launches up)


res = {False: [], True: []}
for _ in range(args.rounds):
    for conv in (False, True):
        res[conv].append(timed(conv))
fmt = lambda m: "%.2f [%.2f .. %.2f]" % (m[len(m) // 2], m[0], m[-1])  # noqa: E731
print("nnet_backward, cnn_tdnn_17f, %d x 1500 frames, natural gradient on, ms: median [min .. max], per round" % args.egs)
for k, kind in enumerate(("updating", "non-updating")):
    for conv in (False, True):
        print("  %-12s conv %-3s " % (kind, "on" if conv else "off") + "  ".join(fmt(r[k]) for r in res[conv])
              + "   | median of the rounds' medians %.2f" % sorted(r[k][len(r[k]) // 2] for r in res[conv])[args.rounds // 2])
net.close()
for b in (fb, og):
    b.free()

# ---- 2. per launch on the model's conv table
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


def clamp(want, dim):
    r = min(want, dim // 2, kf.NG_MAX_RANK)
    return r if r >= 8 else 0


def table(cls, rows):
    t = (cls * len(rows))(*rows)
    return t, kf.upload_f32(np.frombuffer(bytes(t), np.float32))


pres, comps, off, w, h, s, st = [], [], 0, 0, 0, 0, 0
for K, N in convs:
    idx = []
    for D, R in ((K + 1, clamp(80, K + 1)), (N, clamp(80, N))):
        idx.append(len(pres) if R else -1)
        if R:
            Rp = kf.ng_rp(R)
            pres.append(kf.KfNgPre(D, R, w, h, s, st))
            w, h, s, st = w + Rp * D, h + Rp * (kf.ng_w16_ld(D) + 1), s + 2 + Rp, st + kf.ng_stat_offsets(D, R)["floats"]
    comps.append(kf.KfNgComp(off, off + K * N, K, N, idx[0], idx[1]))
    off += (K + 1) * N
ptab, pdev = table(kf.KfNgPre, pres)
ctab, cdev = table(kf.KfNgComp, comps)
opts = kf.KfNgOpts()
kf.core.kf_ng_default_opts(C.byref(opts))
pa = (C.addressof(ptab), pdev.ptr, len(pres))
ta = (C.addressof(ctab), cdev.ptr, len(comps)) + pa
w32, w16, sc = kf.DeviceBuffer(4 * w), kf.DeviceBuffer(2 * h), kf.DeviceBuffer(8 * s)
stat, report = kf.upload_f32(np.zeros(st, np.float32)), kf.upload_f32(np.zeros(len(pres) * kf.NG_REPORT, np.float32))
scratch = kf.DeviceBuffer(kf.core.kf_ng_conv_scratch_bytes(C.addressof(ctab), len(comps), C.addressof(ptab), len(pres)))
sscratch = kf.DeviceBuffer(kf.core.kf_ng_state_scratch_bytes(C.addressof(ptab), len(pres)))
g = kf.upload_f32(rng.standard_normal(off, dtype=np.float32))
kf.check(kf.core.kf_ng_init(*pa, C.byref(opts), w32.ptr, w16.ptr, sc.ptr))
fns = [("kf_ng_conv_stats, non-updating", lambda: kf.check(kf.core.kf_ng_conv_stats(g.ptr, off, *ta, w32.ptr, 4.0, 0, stat.ptr, scratch.ptr))),
       ("kf_ng_conv_stats, updating", lambda: kf.check(kf.core.kf_ng_conv_stats(g.ptr, off, *ta, w32.ptr, 4.0, 1, stat.ptr, scratch.ptr))),
       ("kf_ng_scales", lambda: kf.check(kf.core.kf_ng_scales(*pa, C.byref(opts), sc.ptr, stat.ptr, report.ptr))),
       ("kf_ng_conv_apply", lambda: kf.check(kf.core.kf_ng_conv_apply(g.ptr, off, *ta, w32.ptr, report.ptr, scratch.ptr))),
       ("kf_ng_state, updating", lambda: kf.check(kf.core.kf_ng_state(*pa, C.byref(opts), 1, w32.ptr, w16.ptr, sc.ptr, stat.ptr,
                                                                      sscratch.ptr, report.ptr)))]
print("per launch on the conv table %s (%d preconditioners), us: median [min .. max] of %d"
      % (["%dx%d" % kn for kn in convs], len(pres), args.reps))
for (name, _), (med, lo, hi) in zip(fns, timeit([f for _, f in fns], args.reps)):
    print("  %-32s %8.1f [%.1f .. %.1f]" % (name, med, lo, hi))
