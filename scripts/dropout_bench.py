"""Cost of the TDNN-F per-sequence dropout, which bench.py does not switch on:

1. per launch (HIP events, kf_prof_*): the TDNN-F affine forward and the input-gradient GEMM
   that produces a TDNN-F's dz, on the benchmark's row-subsampled shapes, without and with
   KfEpilogue.drop;
2. the train step of the benchmark model (cnn_tdnn_17f, 64 egs, row-subsampled, chain
   objective, SGD; inputs resident) with dropout-proportion on all 17 tdnnf-layers: the switch
   off and on (p = 0.3), alternating, median and spread of the timed steps (host clock around
   steps that end in a device synchronise).

  python scripts/dropout_bench.py [--egs 64] [--steps 10] [--rounds 3] [--p 0.3]
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
ap.add_argument("--p", type=float, default=0.3)
ap.add_argument("--skip-step", action="store_true")
args = ap.parse_args()

kf.check(kf.core.bridge_gpu_init(0))
rng = np.random.default_rng(0)
FRAMES = 1500
T = args.egs * FRAMES


def dev16(n):
    a = (rng.standard_normal(n) * 0.1).astype(np.float16)
    return kf.upload_fp16(a)


def timeit(fn, reps=20):
    fn()
    kf.sync()
    kf.core.kf_prof_reset()
    kf.core.kf_prof_reserve(4 * reps)
    kf.core.kf_prof_enable(1)
    for _ in range(reps):
        fn()
    kf.sync()
    kf.core.kf_prof_enable(0)
    ms = sorted(r["ms"] for r in kf.prof_records() if r["cls"] == 0)
    kf.core.kf_prof_reset()
    return 1e3 * ms[len(ms) // 2], 1e3 * ms[0], 1e3 * ms[-1]


# ---- 1. per launch: M = the compact rows of T frames, N = 1536, K = 2 x 160
M, N, W = (T - 1) // 3 + 1 + 20, 1536, 160
K = 2 * W
nseg = args.egs
seg = np.minimum(np.arange(M) * 3 // FRAMES, nseg - 1).astype(np.int32)
dseg = kf.DeviceBuffer(M * 4)
kf.check(kf.core.bridge_transfer_int32(dseg.ptr, seg.ctypes.data, M))
tab = kf.upload_f32(rng.uniform(1 - 2 * args.p, 1 + 2 * args.p, (nseg, N)).astype(np.float32))
x, wk, resid = dev16((M + 2) * W), dev16(N * K), dev16(M * N)
y, y2 = kf.DeviceBuffer((M + 2) * N * 2), kf.DeviceBuffer((M + 2) * N * 2)
mask = kf.DeviceBuffer(M * N // 8 + 64)
kf.core.bridge_gpu_memset(mask.ptr, 0x5A, M * N // 8)
bias = dev16(N)
sc, sh = kf.upload_f32(rng.uniform(0.5, 1.5, N).astype(np.float32)), kf.upload_f32(np.zeros(N, np.float32))
rows = []
a_f = kf.operand(x.ptr, W, M, K, 1, nparts=2, part_width=W, tpolicy=1, dt=(0, 1))
b_f = kf.operand(wk.ptr, K, N, K, 1)
a_d = kf.operand(x.ptr, W, M, K, 1, nparts=2, part_width=W, tpolicy=0, dt=(1, 0), edges=[(0, 0, M)])
b_d = kf.operand(wk.ptr, W, N, K, 1, nparts=2, part_width=W, T=2 * N, dt=(0, N))
for drop in (False, True, False, True):
    e = kf.KfEpilogue(out=y.ptr, ldo=N, alpha=1.0, bias=bias.ptr, relu=1, mask_out=mask.ptr, scale=sc.ptr, shift=sh.ptr,
                      resid=resid.ptr, ldr=N, resid_alpha=0.66)
    e2 = kf.KfEpilogue(out=y.ptr, ldo=N, alpha=1.0, resid=resid.ptr, ldr=N, resid_alpha=0.66, out2=y2.ptr, ldo2=N,
                       scale2=sc.ptr, mask_in=mask.ptr)
    if drop:
        for q in (e, e2):
            q.drop, q.ld_drop, q.row_seg = tab.ptr, N, dseg.ptr
    f = lambda: kf.check(kf.core.kf_gemm_fused(M, N, K, C.byref(a_f), C.byref(b_f), C.byref(e)))
    d = lambda: kf.check(kf.core.kf_gemm_fused(M, N, K, C.byref(a_d), C.byref(b_d), C.byref(e2)))
    rows.append(("affine forward  drop=%d" % drop, *timeit(f)))
    rows.append(("input gradient  drop=%d" % drop, *timeit(d)))
print("per launch, M=%d N=%d K=%d (us: median, min, max of 20)" % (M, N, K))
for r in rows:
    print("  %-26s %8.1f %8.1f %8.1f" % r)
if args.skip_step:
    sys.exit(0)

# ---- 2. the train step
xcfg = synth.load_xconfig("cnn_tdnn_17f.xconfig")
lines = [l + " dropout-proportion=0.0" if l.startswith("tdnnf-layer") else l for l in xcfg.splitlines()]
assert sum(l.startswith("tdnnf-layer") for l in lines) == 17
net = kf.Network("\n".join(lines) + "\n", max_frames=T)
synth.init_network(net, seed=42)
assert len(net.dropout_layers()) == 17
net.set_row_subsampling(3)
net.set_sequences(np.arange(args.egs + 1, dtype=np.int32) * FRAMES)
net.set_dropout_proportion(args.p)
P = net.layers[-1][3]
dgraph = chain.DenGraph(synth.make_den_graph(num_pdfs=P))
nbatch = chain.NumBatch(chain.pack_num_fsts([synth.make_num_fst(e, num_pdfs=P) for e in range(args.egs)]))
row0, nfr, stride = synth.chain_layout(args.egs, FRAMES)
objective = chain.Chain(dgraph, max_seqs=args.egs, max_frames=int(nfr.max()))
fb = kf.upload_fp16(synth.make_features(T, 40))
net.forward(fb.ptr, T)
tc, tc0, _ = net.row_set()
assert tc > 0 and stride == 3 and np.all(row0 % 3 == 0)
gbuf = kf.DeviceBuffer(tc * P * 2)
kf.core.bridge_gpu_memset(gbuf.ptr, 0, tc * P * 2)
out_ptr = net.activation("output")[0]


def step():
    net.forward(fb.ptr, T)
    objective.compute(nbatch, out_ptr, P, tc, row0 // 3, nfr, 1, gbuf.ptr, P)
    net.backward(gbuf.ptr)
    net.sgd(1e-8, 0.9)


def timed(on):
    net.set_dropout(on, 1234)
    for _ in range(2):
        step()
    kf.sync()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        step()
        kf.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)


res = {False: [], True: []}
for _ in range(args.rounds):
    for on in (False, True):
        res[on].append(timed(on))
print("train step, %d egs, ms per step (median [min .. max] of %d, per round):" % (args.egs, args.steps))
for on in (False, True):
    print("  dropout %-3s " % ("on" if on else "off") + "  ".join("%.2f [%.2f .. %.2f]" % (m[len(m) // 2], m[0], m[-1])
                                                                  for m in res[on]))
r = objective.result()
print("last objective / frame %.4f (%d of %d egs ok)" % (r.objf / max(r.frames, 1), r.num_ok, args.egs))
