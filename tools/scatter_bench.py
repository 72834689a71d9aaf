#!/usr/bin/env python3
"""Launches the kernels of the scatter correction on one GPU, for a kernel trace:

  scatter_rows_forward_kernel / frame_fft2_columns_kernel<two_gaussians> / scatter_rows_turn_kernel / scatter_rows_inverse_kernel
                         paris_hip_scatter_correction_frames on 1 and on 16 frames of 2048^2 f32 line integrals at margin 24 and 4
                         iterations (padded to 4096^2; the scratch holds one frame, so 16 frames are 16 rounds of 2 * 4 + 1 launches)
                         and of 1024^2 (2048^2; seven frames a round)
  phase_rows_forward_kernel / frame_fft2_columns_kernel<paganin> / phase_rows_inverse_kernel
                         the phase retrieval (paris_hip_phase_retrieval_frames) on the same frames at the same margin: the yardstick

`reps` timed calls each behind 3 warm-up calls, every configuration in a sequence of its own. Prints the wall time per call from a
host clock around the calls and a synchronise; the kernel times come from the trace, summed over the launches of a call. The fused
turn kernel stands against the forward plus the inverse kernel of the same call, which a separate inverse and forward pass per
iteration would launch in its place (and which would store and re-read the scatter on top):

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/scatter_bench.py [--reps 10]
  python tools/scatter_bench.py --summarise <dir> [--reps 10]
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
ITERATIONS = 4
WARM = 3
PITCH_MM = 0.1
SETTING = (0.02, -0.15, 1.0, 0.3, 1.0, 0.5, 0.6, ITERATIONS, MARGIN)     # kernels 3 and 10 pixels of 0.1 mm wide
ALPHA, T_MIN = 0.02, 1e-6                                                # the phase retrieval of tools/phase_bench.py
# launches per round of frames, by the name's part that tells the kernel apart in the trace
KERNELS = {"scatter_rows_forward_kernel": 1, "two_gaussians": ITERATIONS, "scatter_rows_turn_kernel": ITERATIONS - 1,
           "scatter_rows_inverse_kernel": 1, "phase_rows_forward_kernel": 1, "paganin": 1, "phase_rows_inverse_kernel": 1}


def rounds(n, frames):
    """rounds of launches per call: the scratch holds max(1, min(16, 64 MiB / frame spectra)) frames"""
    n_x = 2 * n                                      # n + 48 padded to the next power of two
    per = max(1, min(16, (64 << 20) // (n * (n_x // 2 + 1) * 8)))
    return -(-frames // per)


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for kernel, per_round in KERNELS.items():
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        at = 0
        for n in SIZES:
            for f in FRAMES:
                per_call = rounds(n, f) * per_round
                count = (WARM + reps) * per_call
                mine = us[at:at + count]
                at += count
                if len(mine) != count:
                    raise SystemExit("%s: the trace ends early at %d^2 x %d, %d launches in all (give the run's --reps)" % (kernel, n, f, len(us)))
                calls = sorted(sum(mine[k * per_call:(k + 1) * per_call]) for k in range(WARM, WARM + reps))
                out["%s, %d^2 x %d" % (kernel, n, f)] = {"median_us": round(statistics.median(calls), 3), "min_us": round(calls[0], 3),
                                                         "launches_per_call": per_call,
                                                         "median_us_per_launch": round(statistics.median(mine[WARM * per_call:]), 3)}
        if at != len(us):
            raise SystemExit("%s: %d launches in the trace, %d expected" % (kernel, len(us), at))
    for n in SIZES:
        for f in FRAMES:
            at = ", %d^2 x %d" % (n, f)
            scatter = sum(out[k + at]["median_us"] for k in KERNELS if "scatter" in k or k == "two_gaussians")
            phase = sum(out[k + at]["median_us"] for k in KERNELS if "phase" in k or k == "paganin")
            out["scatter pass" + at] = {"median_us": round(scatter, 3), "per_frame_us": round(scatter / f, 3)}
            out["phase pass" + at] = {"median_us": round(phase, 3), "per_frame_us": round(phase / f, 3)}
            out["turn against forward + inverse, per launch" + at] = {
                "turn_us": out["scatter_rows_turn_kernel" + at]["median_us_per_launch"],
                "forward_plus_inverse_us": round(out["scatter_rows_forward_kernel" + at]["median_us_per_launch"]
                                                 + out["scatter_rows_inverse_kernel" + at]["median_us_per_launch"], 3)}
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

            first = be.wrap_projection(slots.ptr, slots.pitch, n, n)
            stride = slots.pitch * n
            be.set_scatter_correction(SETTING, n, n, PITCH_MM, PITCH_MM)
            out["padded, %d^2" % n] = list(B.scatter_correction_check(SETTING, n, n, PITCH_MM, PITCH_MM))
            for f in FRAMES:
                fill()                              # (repeated correction would run the values away)
                out["scatter wall us, %d^2 x %d" % (n, f)] = timed_calls(be, lambda f=f: be.scatter_correction(first, frame_stride=stride, n_frames=f), args.reps)
            be.clear_scatter_correction()
            be.set_phase_retrieval(ALPHA, T_MIN, MARGIN, n, n, PITCH_MM, PITCH_MM)
            for f in FRAMES:
                fill()
                out["phase wall us, %d^2 x %d" % (n, f)] = timed_calls(be, lambda f=f: be.phase_retrieval(first, frame_stride=stride, n_frames=f), args.reps)
            be.clear_phase_retrieval()
            be.free(slots)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
