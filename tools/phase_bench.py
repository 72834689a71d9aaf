#!/usr/bin/env python3
"""Launches the kernels of the phase retrieval on one GPU, for a kernel trace:

  phase_rows_forward_kernel / frame_fft2_columns_kernel<paganin> / phase_rows_inverse_kernel
                         paris_hip_phase_retrieval_frames on 1 and on 16 frames of 2048^2 f32 line integrals at margin 24 (padded to
                         4096^2; the scratch holds one frame, so 16 frames are 16 rounds of three launches) and of 1024^2 (2048^2; seven
                         frames a round)
  filter_rows_kernel     the row filter (paris_hip_stage_filter) on the same frames, one call per frame: the yardstick

`reps` timed calls each behind 3 warm-up calls, every configuration in a sequence of its own. Prints the wall time per call from a
host clock around the calls and a synchronise; the kernel times come from the trace, summed over the launches of a call:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/phase_bench.py [--reps 10]
  python tools/phase_bench.py --summarise <dir> [--reps 10]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (2048, 1024)
FRAMES = (1, 16)
MARGIN = 24
WARM = 3
ALPHA, T_MIN, PITCH_MM = 0.02, 1e-6, 0.1           # a kernel length of sqrt(alpha) / 2 pi = 0.225 pixels of 0.1 mm
KERNELS = ("phase_rows_forward_kernel", "frame_fft2_columns_kernel", "phase_rows_inverse_kernel")


def rounds(n, frames):
    """launches of each phase kernel per call: the scratch holds max(1, min(16, 64 MiB / frame spectra)) frames"""
    n_x = 2 * n                                      # n + 48 padded to the next power of two
    per = max(1, min(16, (64 << 20) // (n * (n_x // 2 + 1) * 8)))
    return -(-frames // per)


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    configs = [(n, f) for n in SIZES for f in FRAMES]
    for kernel in KERNELS + ("filter_rows_kernel",):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        at = 0
        for n, f in configs:
            per_call = rounds(n, f) if kernel in KERNELS else f
            count = (WARM + reps) * per_call
            mine = us[at:at + count]
            at += count
            if len(mine) != count:
                raise SystemExit("%s: the trace ends early at %d^2 x %d, %d launches in all (give the run's --reps)" % (kernel, n, f, len(us)))
            calls = sorted(sum(mine[k * per_call:(k + 1) * per_call]) for k in range(WARM, WARM + reps))
            out["%s, %d^2 x %d" % (kernel, n, f)] = {"median_us": round(statistics.median(calls), 3), "min_us": round(calls[0], 3),
                                                     "launches_per_call": per_call}
        if at != len(us):
            raise SystemExit("%s: %d launches in the trace, %d expected" % (kernel, len(us), at))
    print(json.dumps(out, indent=1))


def timed_calls(be, call, reps):
    for _ in range(WARM):
        call()
    be.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        call()
    be.synchronize()
    return round((time.perf_counter() - t) * 1e6 / reps, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--summarise")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.reps)
    from paris_amd import backend as B
    out = {}
    with B.Backend(0, synchronous=False) as be:
        for n in SIZES:
            slots = be.make_projection_device(n, n * max(FRAMES))
            assert slots.pitch == 4 * n
            y, x = np.mgrid[0:n, 0:n]
            frame = (0.45 + 0.4 * np.sin(x / 97.0) * np.cos(y / 131.0)).astype(np.float32)

            def fill():
                for k in range(max(FRAMES)):
                    be.upload_raw(frame, be.wrap_projection(slots.ptr + k * slots.pitch * n, slots.pitch, n, n))

            fill()
            first = be.wrap_projection(slots.ptr, slots.pitch, n, n)
            stride = slots.pitch * n
            be.set_phase_retrieval(ALPHA, T_MIN, MARGIN, n, n, PITCH_MM, PITCH_MM)
            out["padded, %d^2" % n] = list(B.phase_retrieval_check(ALPHA, T_MIN, MARGIN, n, n, PITCH_MM, PITCH_MM))
            for f in FRAMES:
                out["phase wall us, %d^2 x %d" % (n, f)] = timed_calls(be, lambda f=f: be.phase_retrieval(first, frame_stride=stride, n_frames=f), args.reps)
            be.clear_phase_retrieval()
            fill()                                  # (repeated filtering would run the values away)
            det = B.DetectorGeometry(n, n, PITCH_MM, PITCH_MM, 0.0, 0.0, 500.0, 500.0, 1.0)

            def filter_frames(f):
                for k in range(f):
                    B.filter(be, be.wrap_projection(slots.ptr + k * stride, slots.pitch, n, n), det)

            for f in FRAMES:
                out["row filter wall us, %d^2 x %d" % (n, f)] = timed_calls(be, lambda f=f: filter_frames(f), args.reps)
            be.free(slots)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
