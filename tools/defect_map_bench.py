#!/usr/bin/env python3
"""Launches the defect-map repair on one GPU, for a kernel trace: a 2048^2 f32 frame on a detector with one dead row, one dead column
and 0.1 % scattered defective pixels, `reps` launches. Prints the plan's counts and the wall time per call from device events; the
kernel time comes from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/defect_map_bench.py [--reps 200]
  python tools/defect_map_bench.py --summarise <dir>     # median / min of the repair kernel's launches in the trace
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

KERNEL = "defect_repair_kernel"


def bench_mask(n=2048):
    rng = np.random.default_rng(1)
    mask = (rng.random((n, n)) < 0.001).astype(np.uint8)
    mask[n // 3, :] = 1
    mask[:, n // 2 + 5] = 1
    return mask


def summarise(directory):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if KERNEL in r["Kernel_Name"]]
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    print(json.dumps({"kernel": KERNEL, "launches": len(us), "median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--summarise", metavar="DIR", help="median from the kernel trace under DIR instead of a run")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch

    from paris_amd import backend as B
    n = 2048
    mask = bench_mask(n)
    frame = (np.random.default_rng(2).random((n, n)) * 3).astype(np.float32)
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    d = be.make_projection_device(n, n)
    be.upload_raw(frame, d)
    info = be.set_defect_map(mask)
    for _ in range(10):
        be.defect_repair_rows(d)
    be.synchronize()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        be.defect_repair_rows(d)
    b.record()
    be.synchronize()
    torch.cuda.synchronize()
    print(json.dumps({"frame": [n, n], "defects": int(info.defects), "unrepairable": int(info.unrepairable), "sources": int(info.sources),
                      "reach_rows": int(info.reach_rows), "plan_bytes": int(info.device_bytes),
                      "us_per_call_wall": round(a.elapsed_time(b) * 1e3 / args.reps, 3)}))
    be.clear_defect_map()
    be.free(d)
    be.close()


if __name__ == "__main__":
    main()
