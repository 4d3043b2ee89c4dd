"""Cost of the training-mode BatchNorm on the conv / prefinal / batchnorm-component sites
(DESIGN.md §27), which bench.py does not switch on. Reported, not gated:

1. per launch (HIP events around each entry on the library stream, entries interleaved) on the
   benchmark model's three conv shapes, rows = egs x 1500, [rows x 2560] fp16 seen as
   [rows H x F] with F = 64, 128, 256: kf_bn_block_stats and kf_bn_block_bwd_stats, beside the
   existing column entry kf_bn_train_stats on the reshaped [rows H x F], ld = F view of the same
   tensor, ops_copy of the same bytes, and the yardstick: kf_bn_train_stats on the TDNN-F shape
   [rows x 1536] in the same call.
2. the block sums of the full [rows x 40 x 64] shape against numpy float64, once: the 64-bit
   index arithmetic no small test reaches.
3. the all-rows train step of configs/cnn_tdnn_17f.xconfig (64 egs, chain objective, SGD; inputs
   resident; row subsampling off, which the mode needs) with the mode on and the sites "tdnnf"
   and "all" alternating: median and spread of the timed steps (host clock around steps that end
   in a device synchronise).

  python scripts/bn_train_sites_bench.py [--egs 64] [--steps 10] [--rounds 3] [--skip-step]
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
FRAMES, W, D = 1500, 2560, 1536
T = args.egs * FRAMES
SHAPES = [(40, 64), (20, 128), (10, 256)]      # (height-out, num-filters-out) of cnn1-2, cnn3-4, cnn5-6

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
tensor = T * W * 2                                          # bytes of one conv activation
# fp16 bit patterns of [0.125, 4): every block's mean is well away from zero, as a ReLU output's
r16 = rng.integers(0x3000, 0x4400, size=(T, W), dtype=np.uint16).view(np.float16)
r = kf.upload_fp16(r16)
g = kf.upload_fp16(rng.integers(0x2000, 0x3000, size=(T, W), dtype=np.uint16).view(np.float16))
out = kf.DeviceBuffer(tensor)
rt = kf.upload_fp16(np.maximum(rng.standard_normal((T, D), dtype=np.float32) + 0.3, 0).astype(np.float16))
FMAX = 1536
st = kf.upload_f32(np.zeros(4 * FMAX, np.float32))
ab = kf.upload_f32(np.zeros(2 * FMAX, np.float32))
acc = kf.upload_f32(np.zeros(2 * (2 + 2 * FMAX), np.float32))
p = lambda k: st.ptr + 4 * FMAX * k  # noqa: E731
accp = (acc.ptr, acc.ptr + 16, acc.ptr + 16 + 8 * FMAX)


def f_block(H, F):
    return lambda: kf.check(kf.core.kf_bn_block_stats(r.ptr, W, T, H, F, 1e-3, 1.0, p(0), p(1), p(2), p(3), *accp))


def f_block_bwd(H, F):
    return lambda: kf.check(kf.core.kf_bn_block_bwd_stats(g.ptr, W, r.ptr, W, T, H, F, p(2), p(3), 1.0, ab.ptr, ab.ptr + 4 * FMAX))


def f_view(H, F):
    return lambda: kf.check(kf.core.kf_bn_train_stats(r.ptr, F, T * H, F, 1e-3, 1.0, p(0), p(1), p(2), p(3), *accp))


def f_yard():
    kf.check(kf.core.kf_bn_train_stats(rt.ptr, D, T, D, 1e-3, 1.0, p(0), p(1), p(2), p(3), *accp))


def f_copy():
    kf.check(kf.core.ops_copy(out.ptr, r.ptr, T * W))


# (the copy first: the yardstick then starts behind a launch that left a tensor of dirty lines to
# drain, §23's observation, and every block entry behind one that only read)
rows = [("ops_copy %dx%d" % (T, W), f_copy, 2 * tensor), ("kf_bn_train_stats %dx%d (yardstick)" % (T, D), f_yard, T * D * 2)]
for H, F in SHAPES:
    rows += [("kf_bn_block_stats H=%d F=%d" % (H, F), f_block(H, F), tensor),
             ("kf_bn_block_bwd_stats H=%d F=%d" % (H, F), f_block_bwd(H, F), 2 * tensor),
             ("kf_bn_train_stats, [%dx%d] view" % (T * H, F), f_view(H, F), tensor)]
res = timeit([f for _, f, _ in rows], args.reps)
print("per entry (us: median, min, max of %d; events around each entry, both launches of a statistics entry inside)" % args.reps)
for (name, _, nbytes), (med, lo, hi) in zip(rows, res):
    print("  %-44s %8.1f %8.1f %8.1f   %6.1f MB -> %5.0f GB/s [%5.0f .. %5.0f]" % (
        name, med, lo, hi, nbytes * 1e-6, nbytes / med * 1e-3, nbytes / hi * 1e-3, nbytes / lo * 1e-3))

# ---- 2. the sums at full size against float64
H, F = SHAPES[0]
kf.core.bridge_gpu_memset(acc.ptr, 0, 8 * (2 + 2 * FMAX))
f_block(H, F)()
a = kf.read_f32(acc.ptr, (2 * (2 + 2 * FMAX),)).view(np.float64)
s_ref, q_ref = np.zeros(F), np.zeros(F)
for i in range(0, T, 4000):
    blk = r16[i:i + 4000].astype(np.float64).reshape(-1, F)
    s_ref += blk.sum(0)
    q_ref += (blk * blk).sum(0)
es = np.max(np.abs(a[2:2 + F] - s_ref) / s_ref)
eq = np.max(np.abs(a[2 + FMAX:2 + FMAX + F] - q_ref) / q_ref)
mean = kf.read_f32(p(0), (F,)).astype(np.float64)
em = np.max(np.abs(mean - s_ref / (T * H)) / (s_ref / (T * H)))
print("block sums at [%d x %d x %d] against numpy float64: count %s (want %d), sum rel err %.2e, sumsq rel err %.2e, "
      "mean rel err %.2e" % (T, H, F, a[0], T * H, es, eq, em))
assert a[0] == T * H and es <= 1e-12 and eq <= 1e-12 and em <= 2.0 ** -23
if args.skip_step:
    sys.exit(0)
for b in (r, g, out, rt):
    b.free()
del r16

# ---- 3. the all-rows train step
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


def timed(sites):
    net.set_batchnorm_train(False)
    net.set_batchnorm_train_sites(sites)
    net.set_batchnorm_train(True)
    for _ in range(2):
        train_step()
    kf.sync()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        train_step()
        kf.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms), len(net.batchnorm_train_layers())


res = {"tdnnf": [], "all": []}
count = {}
for _ in range(args.rounds):
    for sites in ("tdnnf", "all"):
        ms, count[sites] = timed(sites)
        res[sites].append(ms)
print("all-rows train step, cnn_tdnn_17f, %d egs, training-mode BatchNorm on, ms per step (median [min .. max] of %d, per round):"
      % (args.egs, args.steps))
for sites in ("tdnnf", "all"):
    print("  sites %-5s (%2d layers) " % (sites, count[sites])
          + "  ".join("%.2f [%.2f .. %.2f]" % (m[len(m) // 2], m[0], m[-1]) for m in res[sites]))
r_ = objective.result()
print("last objective / frame %.4f (%d of %d egs ok)" % (r_.objf / max(r_.frames, 1), r_.num_ok, args.egs))
