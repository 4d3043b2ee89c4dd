"""Per-kernel resource figures from hipcc's saved temporaries (DESIGN.md §21's table).

Compile the units of interest with --save-temps into a directory per tree, e.g.
  hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 --save-temps -c csrc/gemm_fused.hip -o gemm_fused.o
and run
  python scripts/kernel_resources.py PARENT_DIR BRANCH_DIR
It reads the amdhsa.kernels metadata of every *-gfx950.s: VGPRs, AGPRs, SGPRs, scratch, static
LDS and workgroup size per kernel symbol, lists the symbols of PARENT_DIR whose figures are not
the same in BRANCH_DIR (none: the parent's kernels kept their registers and LDS), and prints the
symbols only BRANCH_DIR has with the occupancy the figures allow: registers are allocated in
granules of 8 per lane out of 512 per SIMD, LDS out of 160 KiB per CU.
"""
import glob
import os
import re
import subprocess
import sys

KEYS = ("vgpr", "agpr", "sgpr", "scratch", "lds", "wg")


def parse(d):
    out = {}
    for f in glob.glob(os.path.join(d, "*-hip-amdgcn-amd-amdhsa-gfx950.s")):
        txt = open(f).read()
        for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\n\.\.\.|\namdhsa\.target)", txt, re.S):
            blk = m.group(0)

            def g(k):
                return re.search(r"\." + k + r":\s*(\S+)", blk).group(1)

            out[g("name")] = dict(vgpr=int(g("vgpr_count")), agpr=int(g("agpr_count")), sgpr=int(g("sgpr_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  wg=int(g("max_flat_workgroup_size")), unit=os.path.basename(f).split("-hip")[0])
    return out


def occupancy(r):
    alloc = (r["vgpr"] + r["agpr"] + 7) // 8 * 8
    waves = min(8, 512 // max(alloc, 1))
    per_wg = max(1, r["wg"] // 64 // 4)          # waves of one workgroup on each SIMD
    return alloc, waves, min(160 * 1024 // max(r["lds"], 1), waves // per_wg)


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        return name


if __name__ == "__main__":
    base, new = parse(sys.argv[1]), parse(sys.argv[2])
    print(len(base), "kernel symbols in", sys.argv[1], "/", len(new), "in", sys.argv[2])
    changed = [k for k in base if k not in new or any(base[k][x] != new[k][x] for x in KEYS)]
    print("symbols of the first tree missing or with other figures in the second:", changed or "none")
    for k in sorted(set(new) - set(base)):
        r = new[k]
        alloc, waves, wgs = occupancy(r)
        print("%-14s %-62s vgpr %3d agpr %2d sgpr %3d scratch %d lds %6d | alloc %3d, %d waves/SIMD, %d workgroups/CU" % (
            r["unit"], re.sub(r"^void ", "", demangle(k)).replace("(anonymous namespace)::", "").split("(")[0][:62], r["vgpr"], r["agpr"], r["sgpr"], r["scratch"],
            r["lds"], alloc, waves, wgs))
