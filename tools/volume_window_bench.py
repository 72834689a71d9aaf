#!/usr/bin/env python3
"""Launches the kernels of the volume export on one GPU, for a kernel trace: a 2048 x 2048 x 256 slab
(4 GiB of fp32 voxels). In this order, `reps` timed calls each behind 3 warm-up calls:

  quantise   paris_hip_volume_quantize, device to device, as u16 and as u8              6 and 5 bytes per voxel
  stats      paris_hip_volume_stats without a histogram and with 4096 bins,             4 bytes per voxel
             on a slab that is 90 % zeros and on one of seeded normal noise

Prints the wall time per call from device events; the kernel times come from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/volume_window_bench.py [--reps 20]
  python tools/volume_window_bench.py --summarise <dir> [--reps 20]   # median / min per case and its achieved bytes/s, beside the
                                                                      # copy rate DESIGN.md section 5 quotes
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = (2048, 2048, 256)
VOXELS = DIMS[0] * DIMS[1] * DIMS[2]
WARM = 3
COPY_TB_PER_S = 6.29   # the measured copy rate of the device
# (kernel, case, bytes per voxel), in launch order per kernel
CASES = (("volume_quantize_kernel", "quantise u16", 6), ("volume_quantize_kernel", "quantise u8", 5),
         ("volume_stats_kernel", "stats, 90 % zeros, no histogram", 4), ("volume_stats_kernel", "stats, 90 % zeros, 4096 bins", 4),
         ("volume_stats_kernel", "stats, noise, no histogram", 4), ("volume_stats_kernel", "stats, noise, 4096 bins", 4))


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {"copy_TB_per_s_quoted": COPY_TB_PER_S, "voxels": VOXELS}
    for kernel in dict.fromkeys(c[0] for c in CASES):
        mine = [c for c in CASES if c[0] == kernel]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        if len(us) != len(mine) * (WARM + reps):
            raise SystemExit("%s: %d launches in the trace, %d cases of %d expected (give the run's --reps)" % (kernel, len(us), len(mine), WARM + reps))
        for k, (_, name, per_voxel) in enumerate(mine):
            timed = sorted(us[k * (WARM + reps) + WARM:(k + 1) * (WARM + reps)])
            med = statistics.median(timed)
            rate = VOXELS * per_voxel / (med * 1e-6) / 1e12
            out[name] = {"median_us": round(med, 1), "min_us": round(timed[0], 1), "bytes": VOXELS * per_voxel, "TB_per_s": round(rate, 3),
                         "of_copy_rate": round(rate / COPY_TB_PER_S, 3)}
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
    air = noise * (torch.rand(VOXELS, dtype=torch.float32, device=dev, generator=gen) < 0.1)   # 90 % zeros
    out_bytes = torch.empty(2 * VOXELS, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    wall = {}

    def timed(name, call):
        for _ in range(WARM):
            call()
        be.synchronize()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            call()
        b.record()
        be.synchronize()
        torch.cuda.synchronize()
        wall[name] = round(a.elapsed_time(b) * 1e3 / args.reps, 1)

    v_noise = be.wrap_volume(noise.data_ptr(), *DIMS, owner=noise)
    v_air = be.wrap_volume(air.data_ptr(), *DIMS, owner=air)
    timed(CASES[0][1], lambda: be.quantize_volume(v_noise, 0.0, 1.0, np.uint16, out=out_bytes.data_ptr()))
    timed(CASES[1][1], lambda: be.quantize_volume(v_noise, 0.0, 1.0, np.uint8, out=out_bytes.data_ptr()))
    for k, v in ((2, v_air), (4, v_noise)):   # (a stats call waits for its result: the wall time includes the copy down and the wait)
        timed(CASES[k][1], lambda: be.volume_stats(v))
        timed(CASES[k + 1][1], lambda: be.volume_stats(v, -1.0, 2.0, 4096))
    counts = be.volume_quantize_counts()
    print(json.dumps({"slab": DIMS, "reps": args.reps, "us_per_call_wall": wall,
                      "quantise_counts": [counts.voxels, counts.below, counts.above, counts.not_finite]}))
    be.close()


if __name__ == "__main__":
    main()
