"""Phase stamps and launch times of the two long-K N = bottleneck products of a TDNN-F layer at
the row-subsampled step's row count, run alone through kf_gemm_fused (kf_gemm_trace):
  fwd   the linear forward:        A = [x(t-s) | x(t)] clamped, scratch-row edge, B = W[K][N]
  dgrad the affine input gradient: A = [dz(t) | dz(t-s)] zero-padded, edge row, B = op_wrows,
        out2 through a row mask, edge_out over rows 0 .. s
Per form: the launch time (HIP events, median of --reps), the traced block's K-step intervals
split into part-0 steps (first touch of a 64-column chunk) and part-1 steps (the same chunk
again), prologue and epilogue. KFP16_LIBDIR selects the build; --tiled 1 switches the
single-staging kernel off where the build has the hook, --force 1 runs it at row counts the
dispatcher leaves to the 384x160 tiles.
usage: python scripts/splice_trace.py [--M 32020] [--N 160] [--pw 1536] [--s 1] [--blk 100]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-fp16_amd", "python"))
import kfp16 as kf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--M", type=int, default=32020)
ap.add_argument("--N", type=int, default=160)
ap.add_argument("--pw", type=int, default=1536)
ap.add_argument("--s", type=int, default=1)
ap.add_argument("--blk", type=int, default=100)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--tiled", type=int, default=0)
ap.add_argument("--force", type=int, default=0, help="1: the single-staging kernel at any row count")
ap.add_argument("--json", default=None)
args = ap.parse_args()
M, N, pw, s = args.M, args.N, args.pw, args.s
K = 2 * pw

kf.check(kf.core.bridge_gpu_init(0))
hook = getattr(kf.core, "kf_gemm_debug_splice_once", None)
if hook is not None:
    hook(0 if args.tiled else 2 if args.force else 1)
rng = np.random.default_rng(5)
x = kf.upload_fp16(rng.standard_normal((M + 1, pw)) * 0.5)
w_mn = kf.upload_fp16(rng.standard_normal((K, N)) / np.sqrt(K))       # forward: W[K][N]
w_rows = kf.upload_fp16(rng.standard_normal((2 * N, pw)) / np.sqrt(K))  # gradient: op_wrows
out = kf.DeviceBuffer((M + 2) * N * 2)
rowmask = np.full((M * N // 8,), 0xFF, np.uint8)
rowmask[(M - 20) * N // 8:(M - 19) * N // 8] = 0
dmask = kf.DeviceBuffer(rowmask.nbytes)
kf.check(kf.core.bridge_transfer_int32(dmask.ptr, rowmask.ctypes.data, rowmask.nbytes // 4), "mask")

forms = {}
A = kf.operand(x.ptr, pw, M, K, 1, nparts=2, part_width=pw, T=M, tpolicy=1, dt=(-s, 0),
               edges=((0, M - 20, M - 1 - s), (1, M - 20, M - 1)))
B = kf.operand(w_mn.ptr, N, K, N, 0)
forms["fwd"] = (A, B, kf.KfEpilogue(out=out.ptr, ldo=N, alpha=1.0))
A = kf.operand(x.ptr, pw, M, K, 1, nparts=2, part_width=pw, T=M, tpolicy=0, dt=(0, -s), edges=((1, M - 1, M),))
B = kf.operand(w_rows.ptr, pw, N, K, 1, nparts=2, part_width=pw, T=2 * N, dt=(0, N))
forms["dgrad"] = (A, B, kf.KfEpilogue(alpha=1.0, out2=out.ptr, ldo2=N, mask_in=dmask.ptr,
                                      edge_out=out.ptr + M * N * 2, edge_r0=0, edge_r1=s + 1, edge_src=1))

nblk = ((M + 127) // 128) * ((N + 159) // 160)
args.blk = min(args.blk, (M + 383) // 384 * ((N + 159) // 160) - 1)
tb = kf.DeviceBuffer((64 + 3 * max(nblk, 4096)) * 8)
result = {"M": M, "N": N, "K": K, "s": s, "tiled": args.tiled, "libdir": os.environ.get("KFP16_LIBDIR", "")}
for name, (A, B, E) in forms.items():
    def run():
        kf.check(kf.core.kf_gemm_fused(M, N, K, C.byref(A), C.byref(B), C.byref(E)), name)
    for _ in range(3):
        run()
    kf.sync()
    kf.core.kf_prof_enable(1)
    kf.core.kf_prof_reserve(args.reps + 4)
    kf.core.kf_prof_reset()
    for _ in range(args.reps):
        run()
    kf.sync()
    recs = [r for r in kf.prof_records() if r["M"] == M]
    kf.core.kf_prof_enable(0)
    us = sorted(1e3 * r["ms"] for r in recs)
    zero = np.zeros((tb.nbytes // 4,), np.int32)
    kf.check(kf.core.bridge_transfer_int32(tb.ptr, zero.ctypes.data, zero.size), "clear")
    kf.core.kf_gemm_trace(tb.ptr, 0, args.blk)
    run()
    kf.sync()
    kf.core.kf_gemm_trace(None, -1, 0)
    a = kf.read_f32(tb.ptr, (tb.nbytes // 4,)).view(np.uint64)  # (a plain 4-byte-word copy)
    p = a[:64].astype(np.float64) * 0.01
    ks = [i for i in range(40) if a[2 + i] > 0]
    iv = np.diff([p[2 + i] for i in ks])  # iv[j]: step ks[j] -> ks[j + 1], the time step ks[j] took
    even, odd = iv[0::2], iv[1::2]
    gx = int(a[61] >> 32)
    rec = a[64:64 + 3 * gx].reshape(gx, 3).astype(np.float64) * 0.01
    dur = rec[:, 1] - rec[:, 0]
    r = {"tile": [int(a[61] & 0xFFFF), int((a[61] >> 16) & 0xFFFF)], "grid": gx,
         "launch_us_median": round(us[len(us) // 2], 2), "launch_us_min_max": [round(us[0], 2), round(us[-1], 2)],
         "block_us_mean": round(float(dur.mean()), 2),
         "prologue_us": round(p[1] - p[0], 2), "first_step_wait_us": round(p[2] - p[1], 2),
         "part0_step_us_mean": round(float(even.mean()), 3), "part1_step_us_mean": round(float(odd.mean()), 3),
         "step_us": [round(float(v), 2) for v in iv],
         "loop_us": round(p[42] - p[1], 2), "epilogue_us": round(p[43] - p[42], 2), "total_us": round(p[43] - p[0], 2)}
    result[name] = r
    print(name, json.dumps(r))
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
