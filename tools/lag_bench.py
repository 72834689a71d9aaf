#!/usr/bin/env python3
"""Launches the kernel of the detector lag correction on one GPU, for a kernel trace:

  lag_kernel<TERMS, true>   the recursive deconvolution in place on n_frames frames of 2048^2 f32 counts, pitch 8192, whole frames,
                            with a flat-field setting in force (its dark is read): per pixel and call 8 n_frames + 8 TERMS + 4 bytes
  flat_field_kernel         paris_hip_flat_field_rows on the same frames: the yardstick, 8 bytes per pixel and frame plus 8 bytes of
                            reference reads per pixel and call

for TERMS = 1 .. 4 and n_frames = 1 and 16. `reps` timed calls each behind 3 warm-up calls, every configuration in a sequence of its
own. Every frame holds the same counts, so that the frames keep their values from call to call (the response has unit DC gain); the
kernel does the same operations whatever they are. Prints the wall time per call from a host clock around the calls and a
synchronise; the kernel times come from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/lag_bench.py [--reps 20]
  python tools/lag_bench.py --summarise <dir> [--reps 20]
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

N = 2048
FRAMES = (1, 16)
TERMS = (1, 2, 3, 4)
WARM = 3
COPY_TB_PER_S = 6.29   # the measured copy rate of the device
MODEL = ((7.1e-6, 2.5e-3), (1.1e-4, 2.1e-2), (1.7e-3, 1.6e-1), (1.9e-2, 1.0))
CONFIGS = [(terms, frames) for frames in FRAMES for terms in TERMS]      # the order of the launches


def lag_bytes(terms, frames):
    return N * N * (8 * frames + 8 * terms + 4)


def flat_bytes(frames):
    return N * N * (8 * frames + 8)


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {"copy_TB_per_s_quoted": COPY_TB_PER_S}

    def medians(kernel, groups):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        per = WARM + reps
        if len(us) != per * len(groups):
            raise SystemExit("%s: %d launches in the trace, %d expected (give the run's --reps)" % (kernel, len(us), per * len(groups)))
        for k, (name, nbytes) in enumerate(groups):
            timed = sorted(us[k * per + WARM:(k + 1) * per])
            med = statistics.median(timed)
            rate = nbytes / (med * 1e-6) / 1e12
            out[name] = {"median_us": round(med, 3), "min_us": round(timed[0], 3), "bytes": nbytes, "TB_per_s": round(rate, 3),
                         "of_copy_rate": round(rate / COPY_TB_PER_S, 3)}

    medians("lag_kernel", [("lag_kernel<%d>, %d frame(s)" % (t, f), lag_bytes(t, f)) for t, f in CONFIGS])
    medians("flat_field_kernel", [("flat_field_kernel, %d frame(s)" % f, flat_bytes(f)) for f in FRAMES])
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--summarise", metavar="DIR", help="medians from the kernel trace under DIR instead of a run")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.reps)
    import torch

    from paris_amd import backend as B
    rng = np.random.default_rng(3)
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    out = {}
    frame = rng.uniform(3000.0, 60000.0, (N, N)).astype(np.float32)
    stack = torch.empty((max(FRAMES), N, N), dtype=torch.float32, device=dev)
    stack.copy_(torch.from_numpy(frame)[None].expand(max(FRAMES), N, N))
    first = be.wrap_projection(stack.data_ptr(), 4 * N, N, N)
    stride = 4 * N * N
    be.set_flat_field(np.full((N, N), 300.0, np.float32), np.full((N, N), 62000.0, np.float32))
    for terms, frames in CONFIGS:
        be.set_lag_correction(MODEL[:terms])
        be.lag_begin(N, N)
        us = timed_calls(be, lambda: be.lag_correct(first, frame_stride=stride, n_frames=frames), args.reps)
        assert be.lag_frames() == (WARM + args.reps) * frames
        be.lag_end()
        out["lag_correct, %d term(s), %d frame(s)" % (terms, frames)] = {"us_per_call_wall": us, "bytes": lag_bytes(terms, frames)}
    be.clear_lag_correction()
    drift = float((stack[0].cpu() - torch.from_numpy(frame)).abs().max())
    for frames in FRAMES:     # last: it turns the counts into line integrals
        stack.copy_(torch.from_numpy(frame)[None].expand(max(FRAMES), N, N))
        us = timed_calls(be, lambda: be.flat_field_rows(first, frame_stride=stride, n_frames=frames), args.reps)
        out["flat_field_rows, %d frame(s)" % frames] = {"us_per_call_wall": us, "bytes": flat_bytes(frames)}
    print(json.dumps({"frame": [N, N], "reps": args.reps, "calls": out, "largest change of a count over all calls": drift}))
    be.clear_flat_field()
    be.close()


if __name__ == "__main__":
    main()
