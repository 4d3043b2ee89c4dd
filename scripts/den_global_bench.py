"""The chain objective alone on the global-rows denominator, which bench.py does not
switch on. Reported, not gated.

64 sequences x 490 frames, the compact stride-1 layout, random fp16 outputs, on two graphs:
  bench  the benchmark graph (S = 7052, P = 3080, A = 113,380): rows="lds" and rows="global"
         alternate call by call in one process: what one launch per frame costs against the
         LDS-resident kernels.
  large  synth.make_den_graph(30000, 600000, 6000), which the LDS path refuses: the time per
         frame against the floor of its record and row bytes at the HBM peak, and the share a
         sequence of minimal launches of the same length takes (2 T + 6 one-element torch adds on
         an idle device, host clock to the synchronise).
A compute is timed by the host clock from the call to the device synchronise; the median of
each round, then the median and the spread of the rounds' medians.

  python scripts/den_global_bench.py [--graph bench|large|both] [--egs 64] [--reps 5] [--rounds 3]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kaldi-fp16_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import kfp16 as kf  # noqa: E402
from kfp16 import chain, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--graph", default="both", choices=["bench", "large", "both"])
ap.add_argument("--egs", type=int, default=64)
ap.add_argument("--frames", type=int, default=490)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
kf.check(kf.core.bridge_gpu_init(0))
B, T = args.egs, args.frames
HBM_PEAK = 8.0e12   # bytes / s


def timed(fn):
    kf.sync()
    t0 = time.perf_counter()
    fn()
    kf.sync()
    return (time.perf_counter() - t0) * 1e3


def rounds(fns):
    """fns: name -> callable; the variants alternate call by call. name -> (median, spread) ms."""
    for f in fns.values():
        f()
    kf.sync()
    meds = {k: [] for k in fns}
    for _ in range(args.rounds):
        ts = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, f in fns.items():
                ts[k].append(timed(f))
        for k in fns:
            meds[k].append(float(np.median(ts[k])))
    return {k: (float(np.median(v)), max(v) - min(v)) for k, v in meds.items()}


def objective(g, rows_mode):
    P = g["P"]
    dg = chain.DenGraph(g, rows=rows_mode)
    nb = chain.NumBatch(chain.pack_num_fsts([synth.make_num_fst(e, num_pdfs=P) for e in range(B)]))
    ch = chain.Chain(dg, max_seqs=B, max_frames=T)
    row0 = (np.arange(B) * T).astype(np.int32)
    fr = np.full(B, T, np.int32)
    x = kf.upload_fp16((np.random.default_rng(3).standard_normal((B * T, P)) * 2).astype(np.float16))
    gbuf = kf.DeviceBuffer(B * T * P * 2)
    o = chain.KfChainOpts.default()
    keep = (dg, nb, ch, x, gbuf)

    def run():
        ch.compute(nb, x.ptr, P, B * T, row0, fr, 1, gbuf.ptr, P, o)
    run.keep, run.ch, run.dg = keep, ch, dg
    return run


if args.graph in ("bench", "both"):
    g = synth.make_den_graph()
    fns = {m: objective(g, m) for m in ("lds", "global")}
    res = rounds(fns)
    r = {m: fns[m].ch.result() for m in fns}
    print("bench graph S=%d P=%d A=%d, %d x %d frames" % (g["S"], g["P"], g["A"], B, T))
    for m, (med, spread) in res.items():
        print("  rows=%-6s %8.3f ms per compute (spread of round medians %.3f), objf %.6f" % (m, med, spread, r[m].objf))

if args.graph in ("large", "both"):
    g = synth.make_den_graph(30000, 600000, 6000)
    run = objective(g, "auto")
    assert run.dg.rows == "global"
    one = torch.zeros(1, device="cuda")
    n_launch = 2 * T + 6

    def empty():
        for _ in range(n_launch):
            one.add_(0.0)
        torch.cuda.synchronize()
    res = rounds({"global": run, "launches": empty})
    nq = min(64, 1 << max(0, (B - 1).bit_length()))
    ngrp = -(-B // nq)
    # per frame: the three tables' records (12 + 8 + 12 B each) once per sequence group; per sequence
    # the alpha and beta rows written once and read once by the posteriors, e written, read by both
    # recursions and replaced by the posteriors, which the assembly reads; the output row in, the
    # gradient row out
    frame_bytes = 32.0 * g["A"] * ngrp + B * (4.0 * 4 * g["S"] + 4.0 * 6 * g["P"] + 4.0 * g["P"])
    floor_ms = frame_bytes * T / HBM_PEAK * 1e3
    med, spread = res["global"]
    lm, _ = res["launches"]
    print("large graph S=%d P=%d A=%d, %d x %d frames, NQ=%d" % (g["S"], g["P"], g["A"], B, T, nq))
    print("  rows=global %8.3f ms per compute (spread %.3f): %.1f us per frame; floor %.3f ms (%.1f MB per frame at "
          "%.0f TB/s) = %.1f %% of the time" % (med, spread, med * 1e3 / T, floor_ms, frame_bytes / 1e6, HBM_PEAK / 1e12,
                                             100 * floor_ms / med))
    print("  %d minimal launches: %.3f ms = %.1f %% of the compute" % (n_launch, lm, 100 * lm / med))
