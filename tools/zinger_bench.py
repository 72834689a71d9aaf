#!/usr/bin/env python3
"""Launches the zinger filter on one GPU, for a kernel trace: a 2048^2 f32 frame (a smooth ramp plus noise) with 0.05 % planted dark
spikes, `reps` calls. Every call starts from the spiked frame again (a device-to-device copy in front of it: the pass is not
idempotent). Prints the counts and the wall time per call from device events; the kernel times come from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/zinger_bench.py [--reps 200]
  python tools/zinger_bench.py --summarise <dir>     # median / min of the two kernels' launches in the trace, and the detect
                                                     # kernel's rate on its 16 MiB of compulsory reads
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

KERNELS = ("zinger_detect_kernel", "zinger_apply_kernel")
N = 2048
T_ABS, SPIKE, SHARE = 0.25, 1.0, 0.0005


def bench_frame(n=N):
    rng = np.random.default_rng(3)
    y, x = np.mgrid[:n, :n]
    f = (1.5 + 0.7 * x / (n - 1) + 0.3 * y / (n - 1) + rng.normal(0, 0.02, (n, n))).astype(np.float32)
    spikes = rng.random((n, n)) < SHARE
    f[spikes] -= np.float32(SPIKE)
    return f, int(spikes.sum())


def summarise(directory):
    out = {}
    for kernel in KERNELS:
        rows = []
        for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
            rows += [r for r in csv.DictReader(open(f)) if kernel in r["Kernel_Name"]]
        us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows)
        us = us[:len(us) - 10] if len(us) > 20 else us   # (the warm-up calls are among the slowest)
        out[kernel] = {"launches": len(rows), "median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3)}
    med = out[KERNELS[0]]["median_us"]
    out["detect_TB_per_s_on_16_MiB"] = round(4.0 * N * N / (med * 1e-6) / 1e12, 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--summarise", metavar="DIR", help="medians from the kernel trace under DIR instead of a run")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch

    from paris_amd import backend as B
    frame, planted = bench_frame()
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    work = torch.empty((N, N), dtype=torch.float32, device=dev)
    src = torch.empty((N, N), dtype=torch.float32, device=dev)
    src.copy_(torch.from_numpy(frame))
    w = be.wrap_projection(work.data_ptr(), 4 * N, N, N)
    be.set_zinger_filter(T_ABS, 0.0, "dark", N, N)
    for _ in range(10):
        work.copy_(src)
        be.zinger_filter_rows(w)
    be.synchronize()
    torch.cuda.synchronize()
    be.zinger_stats(reset=True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        work.copy_(src)
        be.zinger_filter_rows(w)
    b.record()
    be.synchronize()
    torch.cuda.synchronize()
    st = be.zinger_stats()
    print(json.dumps({"frame": [N, N], "planted": planted, "frames": int(st.frames), "replaced_per_frame": int(st.replaced) / max(1, int(st.frames)),
                      "saturated_frames": int(st.saturated_frames), "us_per_call_wall_with_copy": round(a.elapsed_time(b) * 1e3 / args.reps, 3)}))
    be.clear_zinger_filter()
    be.close()


if __name__ == "__main__":
    main()
