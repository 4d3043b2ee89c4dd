"""Cost of SpecAugment, which bench.py's config has no layer for. Reported, not
gated:

1. per launch (HIP events around each launch on the library stream): kf_specaug_rows and
   kf_specaug_apply on T = egs x 1500 frames of 40 columns, one sequence per eg, m = 20, z = 0.2,
   f = 0.5, and next to kf_specaug_apply in the same call ops_copy of the same tensor: the HBM
   yardstick of a pass that reads and writes [T x 40] fp16. The ratio apply / copy is printed.
2. the train step of configs/specaug/cnn_tdnn_17f_kaldi_specaug.xconfig (64 egs, ivector front end, xent branch,
   row-subsampled, chain objective, SGD; inputs resident) with the switch off and on,
   alternating: median and spread of the timed steps (host clock around steps that end in a
   device synchronise).

  python scripts/specaug_bench.py [--egs 64] [--steps 10] [--rounds 3] [--skip-step]
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
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--skip-step", action="store_true")
args = ap.parse_args()

kf.check(kf.core.bridge_gpu_init(0))
FRAMES, D = 1500, 40
T, B = args.egs * FRAMES, args.egs
M_, Z_, F_ = 20, 0.2, 0.5

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
    """us per launch of each fn: HIP events around every launch, the fns interleaved (median, min, max)"""
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
seq = (np.arange(B + 1, dtype=np.int32) * FRAMES)
dso = kf.DeviceBuffer((B + 1) * 4)
kf.check(kf.core.bridge_transfer_int32(dso.ptr, seq.ctypes.data, B + 1))
rows = kf.DeviceBuffer(T * 4)
x = kf.upload_fp16((np.random.default_rng(0).standard_normal((T, D))).astype(np.float16))
y, y2 = kf.DeviceBuffer(T * D * 2), kf.DeviceBuffer(T * D * 2)
Zb = min(D, int(D * F_ + 0.5))
m_n = max(1, int(M_ * (1.0 - Z_) / Z_))
step = [0]


def f_rows():
    kf.check(kf.core.kf_specaug_rows(rows.ptr, dso.ptr, B, T, D, Zb, Z_, M_, m_n, 0, 1234, step[0] & 0xFFFF))
    step[0] += 1


def f_apply():
    kf.check(kf.core.kf_specaug_apply(x.ptr, D, y.ptr, D, T, D, rows.ptr))


def f_copy():
    kf.check(kf.core.ops_copy(y2.ptr, x.ptr, T * D))


(r_med, r_min, r_max), (a_med, a_min, a_max), (c_med, c_min, c_max) = timeit([f_rows, f_apply, f_copy], args.reps)
nbytes = 2 * T * D * 2
zeroed = float(np.mean(kf.read_f32(rows.ptr, (T,)).view(np.int32) == -1))
print("per launch, T=%d B=%d dim=%d m=%d z=%g f=%g (us: median, min, max of %d; events around each launch)"
      % (T, B, D, M_, Z_, F_, args.reps))
print("  %-18s %8.1f %8.1f %8.1f" % ("kf_specaug_rows", r_med, r_min, r_max))
print("  %-18s %8.1f %8.1f %8.1f   (%.0f GB/s of the %d bytes a full read + write moves; %.1f%% of rows zeroed, not read)"
      % ("kf_specaug_apply", a_med, a_min, a_max, nbytes / a_med * 1e-3, nbytes, 100 * zeroed))
print("  %-18s %8.1f %8.1f %8.1f   (%.0f GB/s)" % ("ops_copy", c_med, c_min, c_max, nbytes / c_med * 1e-3))
print("  apply / copy = %.2f (medians), %.2f (minima)" % (a_med / c_med, a_min / c_min))
if args.skip_step:
    sys.exit(0)

# ---- 2. the train step
net = kf.Network(synth.load_xconfig("specaug/cnn_tdnn_17f_kaldi_specaug.xconfig"), max_frames=T)
synth.init_network(net, seed=42)
assert net.spec_augment_layers() == ["idct-spec-augment"]
net.set_row_subsampling(3)
names = [n for n, *_ in net.layers]
P = net.layers[names.index("output")][3]
dgraph = chain.DenGraph(synth.make_den_graph(num_pdfs=P))
nbatch = chain.NumBatch(chain.pack_num_fsts([synth.make_num_fst(e, num_pdfs=P) for e in range(args.egs)]))
row0, nfr, stride = synth.chain_layout(args.egs, FRAMES)
objective = chain.Chain(dgraph, max_seqs=args.egs, max_frames=int(nfr.max()))
fb = kf.upload_fp16(synth.make_features(T, 40))
ib = kf.upload_fp16((np.random.default_rng(99).standard_normal((B, 100)) * 2).astype(np.float16))
net.forward_ivector(fb.ptr, T, ib.ptr, seq)
tc, tc0, _ = net.row_set()
assert tc > 0 and stride == 3 and np.all(row0 % 3 == 0)
gbuf = kf.DeviceBuffer(tc * P * 2)
kf.core.bridge_gpu_memset(gbuf.ptr, 0, tc * P * 2)
out_ptr = net.activation("output")[0]


def train_step():
    net.forward_ivector(fb.ptr, T, ib.ptr, seq)
    objective.compute(nbatch, out_ptr, P, tc, row0 // 3, nfr, 1, gbuf.ptr, P)
    net.backward(gbuf.ptr)
    net.sgd(1e-8, 0.9)


def timed(on):
    net.set_spec_augment(on, 1234)
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
print("train step, cnn_tdnn_17f_kaldi_specaug, %d egs, ms per step (median [min .. max] of %d, per round):" % (args.egs, args.steps))
for on in (False, True):
    print("  SpecAugment %-3s " % ("on" if on else "off") + "  ".join("%.2f [%.2f .. %.2f]" % (m[len(m) // 2], m[0], m[-1])
                                                                      for m in res[on]))
rb = net.spec_augment_rows("idct-spec-augment")
print("last step: %.1f%% of the frames zeroed, mean band width %.1f of %d" % (100 * np.mean(rb == -1), np.mean(rb[rb != -1] >> 16), D))
r = objective.result()
print("last objective / frame %.4f (%d of %d egs ok)" % (r.objf / max(r.frames, 1), r.num_ok, args.egs))
