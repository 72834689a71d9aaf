#!/usr/bin/env python3
"""Launches the two passes of the ring filter on one GPU, for a kernel trace: 2048^2 f32 frames (a smooth ramp plus noise), 48 of them
one under the other. In this order, `reps` timed calls each behind 10 warm-up calls:

  accumulate   paris_hip_ring_profile_add_rows with 1, 8 and 48 frames per call      4 n + 16 bytes per pixel and call
  subtract     paris_hip_ring_correct_rows on one frame, c != 0 in every pixel       12 bytes per pixel
               and c != 0 in 3 % of the pixels                                        4 bytes per pixel + 8 per corrected pixel
  flat field   paris_hip_flat_field_rows on one frame and on the 48, the same frames  16 bytes per pixel (4 + 4 and the two references)

Prints the wall time per call from device events; the kernel times come from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/ring_bench.py [--reps 100]
  python tools/ring_bench.py --summarise <dir> [--reps 100]   # median / min per case and its achieved bytes/s, beside the copy rate
                                                              # DESIGN.md section 5 quotes
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
SHARE = 0.03
COPY_TB_PER_S = 6.29   # the measured copy rate of the device
# (kernel, case, frames per call, bytes per pixel and frame of the call, bytes per pixel and call), in launch order per kernel
CASES = (("ring_accumulate_kernel", "accumulate 1 frame", 1, 4, 16), ("ring_accumulate_kernel", "accumulate 8 frames", 8, 4, 16),
         ("ring_accumulate_kernel", "accumulate 48 frames", 48, 4, 16),
         ("ring_subtract_kernel", "subtract, every pixel", 1, 12, 0), ("ring_subtract_kernel", "subtract, 3 % of the pixels", 1, 8 * SHARE, 4),
         ("flat_field_kernel", "flat field 1 frame", 1, 16, 0), ("flat_field_kernel", "flat field 48 frames", 48, 16, 0))


def case_bytes(frames, per_frame, per_call):
    return N * N * (frames * per_frame + per_call)


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {"copy_TB_per_s_quoted": COPY_TB_PER_S}
    for kernel in dict.fromkeys(c[0] for c in CASES):
        mine = [c for c in CASES if c[0] == kernel]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        if len(us) != len(mine) * (WARM + reps):
            raise SystemExit("%s: %d launches in the trace, %d cases of %d expected (give the run's --reps)" % (kernel, len(us), len(mine), WARM + reps))
        for k, (_, name, frames, per_frame, per_call) in enumerate(mine):
            timed = sorted(us[k * (WARM + reps) + WARM:(k + 1) * (WARM + reps)])
            med = statistics.median(timed)
            rate = case_bytes(frames, per_frame, per_call) / (med * 1e-6) / 1e12
            out[name] = {"median_us": round(med, 3), "min_us": round(timed[0], 3), "bytes": int(case_bytes(frames, per_frame, per_call)),
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
    dense = np.full((N, N), 0.01, np.float32)
    sparse = np.where(rng.random((N, N)) < SHARE, np.float32(0.01), np.float32(0))
    flat = (2.0 + rng.random((N, N))).astype(np.float32) * 4
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    stack = torch.empty((FRAMES, N, N), dtype=torch.float32, device=dev)
    stack.copy_(torch.from_numpy(frame)[None].expand(FRAMES, N, N))
    first = be.wrap_projection(stack.data_ptr(), 4 * N, N, N)
    stride = 4 * N * N
    out = {}

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
        out[name] = round(a.elapsed_time(b) * 1e3 / args.reps, 3)

    be.ring_profile_begin(N, N)
    for _, name, frames, _, _ in CASES[:3]:
        timed(name, lambda: be.ring_profile_add_rows(first, frame_stride=stride, n_frames=frames))
    be.ring_profile_discard()
    for (_, name, _, _, _), c in zip(CASES[3:5], (dense, sparse)):
        be.set_ring_correction(c)
        timed(name, lambda: be.ring_correct_rows(first))
    be.clear_ring_correction()
    be.set_flat_field(None, flat)
    for _, name, frames, _, _ in CASES[5:]:   # (the frames turn into other numbers call after call: the pass costs the same)
        timed(name, lambda: be.flat_field_rows(first, frame_stride=stride, n_frames=frames))
    be.clear_flat_field()
    print(json.dumps({"frame": [N, N], "reps": args.reps, "us_per_call_wall": out}))
    be.close()


if __name__ == "__main__":
    main()
