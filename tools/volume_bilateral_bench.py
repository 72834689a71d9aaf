#!/usr/bin/env python3
"""Launches the 3-D bilateral filter on one GPU, for a kernel trace: a 2048 x 2048 x 256 slab (4 GiB of fp32
voxels, seeded normal noise of 0.3 around 0.5, sigma_r = 0.3, sigma_s = 1.25) filtered whole into a second buffer. In this order,
`reps` timed calls each behind 3 warm-up calls: radius 1, 2 and 3 (27, 125 and 343 taps per voxel).

Prints the wall time per call from device events; the kernel times come from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/volume_bilateral_bench.py [--reps 20]
  python tools/volume_bilateral_bench.py --summarise <dir> [--reps 20]

The summary puts each median beside three bounds computed here:
  copy   the slab's 8 bytes per voxel (4 read, 4 written) at the copy rate DESIGN.md section 5 quotes;
  valu   the vector instructions of the inner tap -- counted in the ISA listing of the product build's dz loop body, which holds
         (2r + 1)^2 taps of the 4 (r = 3: 2) outputs of a lane -- times the taps, at one wave instruction per 2 cycles and SIMD: 4 SIMDs on each of
         256 CUs at 2.4 GHz issue 1.2288e12 wave instructions a second;
  lds    the LDS reads of the inner tap, likewise counted (the range gather and the share of the neighbour and spatial reads that
         registers do not keep), at the 75 TB/s the device sustains for conflict-free ds_read_b32 -- the gather's bank conflicts
         come on top.
PARIS_HIP_LIBRARY names another build of the library; with the experiments build PARIS_BILATERAL_TILE_Y=8 or 16 forces the tile
height for every radius (the A/B arms; the counts above are the product's)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = (2048, 2048, 256)
VOXELS = DIMS[0] * DIMS[1] * DIMS[2]
WARM = 3
RADII = (1, 2, 3)
SIGMA_R, SIGMA_S = 0.3, 1.25
COPY_TB_PER_S = 6.29            # the measured copy rate of the device
WAVE_INSTRUCTIONS_PER_S = 256 * 4 * 2.4e9 / 2
LDS_B32_TB_PER_S = 75.0
# per tap and output, from the ISA listing of volume_bilateral_kernel<R>'s dz loop body (hipcc --offload-arch=gfx950 -S, product flags):
# v_* and ds_read* instructions over (2r + 1)^2 * 4 (r = 3: * 2) tap evaluations (a ds_read2_b32 counts once: it is one wave instruction of two dwords)
VALU_PER_TAP = {1: 12.28, 2: 12.24, 3: 12.55}   # sub, 3 mul, cmp, cvt, shift, 2 add, 3 select, and the loop's few address adds
LDS_READS_PER_TAP = {1: 1.39, 2: 1.33, 3: 1.54}


def bounds(r):
    taps = (2 * r + 1) ** 3
    return {"copy_us": VOXELS * 8 / (COPY_TB_PER_S * 1e12) * 1e6,
            "valu_us": VALU_PER_TAP[r] * taps * VOXELS / 64 / WAVE_INSTRUCTIONS_PER_S * 1e6,
            "lds_us": LDS_READS_PER_TAP[r] * taps * VOXELS * 4 / (LDS_B32_TB_PER_S * 1e12) * 1e6}


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "volume_bilateral_kernel" in r["Kernel_Name"]]
    if len(us) != len(RADII) * (WARM + reps):
        raise SystemExit("%d launches in the trace, %d cases of %d expected (give the run's --reps)" % (len(us), len(RADII), WARM + reps))
    out = {"voxels": VOXELS, "copy_TB_per_s_quoted": COPY_TB_PER_S}
    for k, r in enumerate(RADII):
        timed = sorted(us[k * (WARM + reps) + WARM:(k + 1) * (WARM + reps)])
        med = statistics.median(timed)
        b = bounds(r)
        binding = max(b, key=b.get)
        out["radius %d" % r] = {"taps": (2 * r + 1) ** 3, "median_us": round(med, 1), "min_us": round(timed[0], 1), "max_us": round(timed[-1], 1),
                                "GVoxel_per_s": round(VOXELS / med / 1e3, 2), "bounds_us": {n: round(v, 1) for n, v in b.items()},
                                "binding": binding, "times_the_binding_bound": round(med / b[binding], 2)}
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--summarise", metavar="DIR", help="medians from the kernel trace under DIR instead of a run")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.reps)
    import torch

    from paris_amd import backend as B
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    noise = torch.randn(VOXELS, dtype=torch.float32, device=dev, generator=gen) * 0.3 + 0.5
    out = torch.empty(VOXELS, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    v = be.wrap_volume(noise.data_ptr(), *DIMS, owner=noise)
    wall = {}
    for r in RADII:
        be.set_volume_bilateral(SIGMA_R, SIGMA_S, r)
        for _ in range(WARM):
            be.volume_bilateral(v, out=out.data_ptr())
        be.synchronize()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            be.volume_bilateral(v, out=out.data_ptr())
        b.record()
        be.synchronize()
        torch.cuda.synchronize()
        wall["radius %d" % r] = round(a.elapsed_time(b) * 1e3 / args.reps, 1)
    print(json.dumps({"slab": DIMS, "reps": args.reps, "sigma_r": SIGMA_R, "sigma_s": SIGMA_S, "us_per_call_wall": wall,
                      "std_in": round(float(noise[:1 << 24].std()), 4), "std_out_radius_3": round(float(out[:1 << 24].std()), 4)}))
    be.close()


if __name__ == "__main__":
    main()
