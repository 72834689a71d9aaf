#!/usr/bin/env python3
"""Launches the kernels of the beam-hardening correction on one GPU, for a kernel trace:

  bh_apply_kernel      the polynomial (degree 3) in place on 48 frames of 2048^2 f32, pitch 8192       8 bytes per pixel
  flat_field_kernel    paris_hip_flat_field_rows on the same buffer: the yardstick, 8 bytes per pixel of the frames (its two
                       reference frames, 32 MiB, stay in cache)
  bh_classify_kernel   the labels of a 2048 x 2048 x 32 slab, margin 2                                  4 bytes read + 1 written per voxel
  bh_gram_kernel       the Gram sums of N = 2 basis slabs of that size over those labels               9 bytes per voxel
  bh_gram_fold_kernel  the fold of its 65536 partial sums of 6 terms                                    3 MiB

`reps` timed calls each behind 3 warm-up calls. The coefficients are (1, 0, 0), so that the frames keep their values from call to
call; the kernel does the same operations whatever they are. Prints the wall time per call from a host clock around the calls and
a synchronise; the kernel times come from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/beam_hardening_bench.py [--reps 20]
  python tools/beam_hardening_bench.py --summarise <dir> [--reps 20]
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
FRAMES = 48
SLICES = 32
WARM = 3
COPY_TB_PER_S = 6.29   # the measured copy rate of the device
VOXELS = N * N * SLICES
# (kernel, bytes per launch)
KERNELS = (("bh_apply_kernel", FRAMES * N * N * 8), ("flat_field_kernel", FRAMES * N * N * 8), ("bh_classify_kernel", VOXELS * 5),
           ("bh_gram_kernel", VOXELS * 9), ("bh_gram_fold_kernel", 65536 * 6 * 8))


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {"copy_TB_per_s_quoted": COPY_TB_PER_S}
    for kernel, nbytes in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        if len(us) != WARM + reps:
            raise SystemExit("%s: %d launches in the trace, %d expected (give the run's --reps)" % (kernel, len(us), WARM + reps))
        timed = sorted(us[WARM:])
        med = statistics.median(timed)
        rate = nbytes / (med * 1e-6) / 1e12
        out[kernel] = {"median_us": round(med, 3), "min_us": round(timed[0], 3), "bytes": nbytes, "TB_per_s": round(rate, 3),
                       "of_copy_rate": round(rate / COPY_TB_PER_S, 3)}
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
    # the pass beside the flat-field pass, on one buffer
    frame = rng.uniform(0.5, 2.5, (N, N)).astype(np.float32)
    stack = torch.empty((FRAMES, N, N), dtype=torch.float32, device=dev)
    stack.copy_(torch.from_numpy(frame)[None].expand(FRAMES, N, N))
    first = be.wrap_projection(stack.data_ptr(), 4 * N, N, N)
    stride = 4 * N * N
    be.set_beam_hardening([1.0, 0.0, 0.0], N, N)
    be.set_flat_field(None, np.full((N, N), 4.0, np.float32))
    out["beam_hardening, 48 frames"] = timed_calls(be, lambda: be.beam_hardening(first, frame_stride=stride, n_frames=FRAMES), args.reps)
    out["flat_field_rows, 48 frames"] = timed_calls(be, lambda: be.flat_field_rows(first, frame_stride=stride, n_frames=FRAMES), args.reps)
    be.clear_beam_hardening()
    be.clear_flat_field()
    del stack
    # the fit's two kernels on a slab: a cylinder of object in noisy air, f_2 its square
    y, x = np.mgrid[:N, :N]
    disc = ((x - N / 2) ** 2 + (y - N / 2) ** 2 < (0.35 * N) ** 2)
    slice_ = (np.where(disc, 0.2, 0.0) + rng.normal(0, 0.005, (N, N))).astype(np.float32)
    f1 = torch.empty((SLICES, N, N), dtype=torch.float32, device=dev)
    f1.copy_(torch.from_numpy(slice_)[None].expand(SLICES, N, N))
    f2 = f1 * f1
    torch.cuda.synchronize()
    v1, v2 = be.wrap_volume(f1.data_ptr(), N, N, SLICES, owner=f1), be.wrap_volume(f2.data_ptr(), N, N, SLICES, owner=f2)
    labels = be.make_labels_device(N, N, SLICES)
    out["bh_classify"] = timed_calls(be, lambda: be.bh_classify(v1, 0.1, 2, labels=labels), args.reps)
    result = []
    out["bh_gram (synchronous: two kernels, two copies, an allocation)"] = timed_calls(be, lambda: result.append(be.bh_gram([v1, v2], labels)), args.reps)
    counts = result[-1][1]
    print(json.dumps({"frame": [N, N], "frames": FRAMES, "slab": [N, N, SLICES], "reps": args.reps, "us_per_call_wall": out,
                      "n_object": counts.n_object, "n_air": counts.n_air, "n_ignored": counts.n_ignored}))
    be.free(labels)
    be.close()


if __name__ == "__main__":
    main()
