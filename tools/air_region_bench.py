#!/usr/bin/env python3
"""Launches the two kernels of the air-region normalisation on one GPU, for a kernel trace: 2048^2 f32 frames (a smooth ramp plus
noise), 48 of them one under the other, the rectangle 64 columns by 2048 rows at the frame's left edge. `reps` timed calls of
paris_hip_air_normalize_rows each behind 10 warm-up calls, with 1 and with 48 frames per call:

  air_value_kernel      one workgroup per frame reads the rectangle and its mask bytes     5 bytes per pixel of the rectangle
  air_subtract_kernel   p <- p - a_f over the whole frame                                   8 bytes per pixel of the frame

A constant is added to the frames before every call (a torch kernel, not counted), so that no call finds the value 0 the call
before left behind and skips its frames. Prints the wall time per call from device events, that addition included; the kernel times
come from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/air_region_bench.py [--reps 100]
  python tools/air_region_bench.py --summarise <dir> [--reps 100]   # median / min per case and its achieved bytes/s, beside the copy
                                                                    # rate DESIGN.md section 5 quotes
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

N = 2048
FRAMES = 48
WARM = 10
RECT = (0, 0, 64, N)
COPY_TB_PER_S = 6.29   # the measured copy rate of the device
PER_CALL = (1, FRAMES)
# (kernel, bytes per frame)
KERNELS = (("air_value_kernel", RECT[2] * RECT[3] * 5), ("air_subtract_kernel", N * N * 8))


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {"copy_TB_per_s_quoted": COPY_TB_PER_S}
    for kernel, per_frame in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        if len(us) != len(PER_CALL) * (WARM + reps):
            raise SystemExit("%s: %d launches in the trace, %d cases of %d expected (give the run's --reps)" % (kernel, len(us), len(PER_CALL), WARM + reps))
        for k, frames in enumerate(PER_CALL):
            timed = sorted(us[k * (WARM + reps) + WARM:(k + 1) * (WARM + reps)])
            med = statistics.median(timed)
            rate = frames * per_frame / (med * 1e-6) / 1e12
            out["%s, %d frame(s)" % (kernel, frames)] = {"median_us": round(med, 3), "min_us": round(timed[0], 3), "bytes": frames * per_frame,
                                                         "TB_per_s": round(rate, 3), "of_copy_rate": round(rate / COPY_TB_PER_S, 3)}
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--summarise", metavar="DIR", help="medians from the kernel trace under DIR instead of a run")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.reps)
    import torch

    from paris_amd import backend as B
    rng = np.random.default_rng(3)
    y, x = np.mgrid[:N, :N]
    frame = (1.5 + 0.7 * x / (N - 1) + 0.3 * y / (N - 1) + rng.normal(0, 0.02, (N, N))).astype(np.float32)
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    stack = torch.empty((FRAMES, N, N), dtype=torch.float32, device=dev)
    stack.copy_(torch.from_numpy(frame)[None].expand(FRAMES, N, N))
    first = be.wrap_projection(stack.data_ptr(), 4 * N, N, N)
    stride = 4 * N * N
    be.set_air_region(*RECT, N, N)
    out = {}
    for frames in PER_CALL:
        def call():
            stack[:frames].add_(0.25)
            be.air_normalize(first, frame_stride=stride, n_frames=frames)

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
        out["%d frame(s) per call" % frames] = round(a.elapsed_time(b) * 1e3 / args.reps, 3)
    st = be.air_stats()
    be.clear_air_region()
    print(json.dumps({"frame": [N, N], "rectangle": RECT, "reps": args.reps, "us_per_call_wall_with_the_addition": out,
                      "frames": st.frames, "normalised": st.normalised}))
    be.close()


if __name__ == "__main__":
    main()
