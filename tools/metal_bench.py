#!/usr/bin/env python3
"""Launches the kernels of the metal artefact reduction on one GPU, for a kernel trace:

  metal_inpaint_kernel   paris_hip_metal_inpaint_rows on 1 and on 16 frames of 2048^2 f32 line integrals (pitch 8192, whole frames)
                         with an EMPTY trace -- the pass reads the frames' words, 1/32 of their bytes, and nothing else -- and with a
                         trace of two discs per frame that covers about 3 % of the pixels
  zinger_detect_kernel   paris_hip_zinger_filter_rows on the same frames: the yardstick (with zinger_apply_kernel)
  metal_pack_kernel      paris_hip_metal_trace_pack of 16 frames of 2048^2 (grow 1): the unit the driver packs 1440 views in
  metal_count / _scan / _write / _binarize_kernel   paris_hip_metal_collect of a 1024^3 volume with binarize, 1e-4 of the voxels hit

`reps` timed calls each behind 3 warm-up calls, every configuration in a sequence of its own. Prints the wall time per call from a
host clock around the calls and a synchronise; the kernel times come from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/metal_bench.py [--reps 10]
  python tools/metal_bench.py --summarise <dir> [--reps 10]
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
WARM = 3
VOLUME = 1024
HIT_FRACTION = 1e-4


def disc_trace(n_views):
    """packed traces of n_views frames: two discs of radius 140 pixels per frame, 2 pi 140^2 / 2048^2 = 2.9 % of the pixels"""
    y, x = np.mgrid[0:N, 0:N]
    one = ((x - 700) ** 2 + (y - 900) ** 2 < 140 ** 2) | ((x - 1400) ** 2 + (y - 1100) ** 2 < 140 ** 2)
    words = np.packbits(one.reshape(N, N // 64, 64), axis=-1, bitorder="little").view(np.uint64).reshape(N, N // 64)
    return np.broadcast_to(words, (n_views, N, N // 64)).copy(), float(one.mean())


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}

    def medians(kernel, names, launches_per_call=1):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        per = (WARM + reps) * launches_per_call
        if len(us) != per * len(names):
            raise SystemExit("%s: %d launches in the trace, %d expected (give the run's --reps)" % (kernel, len(us), per * len(names)))
        for k, name in enumerate(names):
            timed = sorted(us[k * per + WARM * launches_per_call:(k + 1) * per])
            out["%s, %s" % (kernel, name)] = {"median_us": round(statistics.median(timed), 3), "min_us": round(timed[0], 3)}

    frames = ["%d frame(s)" % f for f in FRAMES]
    medians("metal_inpaint_kernel", ["empty trace, " + f for f in frames] + ["3 % trace, " + f for f in frames])
    medians("zinger_detect_kernel", frames)
    medians("zinger_apply_kernel", frames)
    medians("metal_pack_kernel", ["16 frames"])
    for k in ("metal_count_kernel", "metal_scan_kernel", "metal_write_kernel", "metal_binarize_kernel"):
        medians(k, ["%d^3" % VOLUME])
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
    rng = np.random.default_rng(1)
    with B.Backend(0, synchronous=False) as be:
        slots = be.make_projection_device(N, N * max(FRAMES))
        assert slots.pitch == 4 * N
        # a smooth frame with 0.05 % dark spikes (2 074 per frame, the zinger benchmark's share): few pixels for the yardstick to flag
        y, x = np.mgrid[0:N, 0:N]
        frame = (0.45 + 0.4 * np.sin(x / 97.0) * np.cos(y / 131.0)).astype(np.float32)
        frame.reshape(-1)[rng.choice(N * N, 2074, replace=False)] -= np.float32(1.0)
        for k in range(max(FRAMES)):
            be.upload_raw(frame, be.wrap_projection(slots.ptr + k * slots.pitch * N, slots.pitch, N, N))
        first = be.wrap_projection(slots.ptr, slots.pitch, N, N)
        stride = slots.pitch * N
        discs, share = disc_trace(max(FRAMES))
        out["trace_share"] = round(share, 4)
        for label, bits in (("empty trace", np.zeros_like(discs)), ("3 % trace", discs)):
            be.set_metal_trace(bits, N)
            for f in FRAMES:
                out["inpaint wall us, %s, %d frame(s)" % (label, f)] = timed_calls(
                    be, lambda f=f: be.metal_inpaint(first, view=list(range(f)), frame_stride=stride, n_frames=f), args.reps)
        be.clear_metal_trace()
        be.set_zinger_filter(0.25, 0.0, 0, N, N)
        for f in FRAMES:
            out["zinger wall us, %d frame(s)" % f] = timed_calls(be, lambda f=f: be.zinger_filter_rows(first, frame_stride=stride, n_frames=f), args.reps)
        be.clear_zinger_filter()
        # pack: the frames hold values up to 0.85; above 0.8 is a hit
        out["pack wall us, 16 frames"] = timed_calls(be, lambda: be.metal_trace_pack(first, 0.8, 1, frame_stride=stride, n_frames=16), args.reps)
        be.free(slots)
        v = be.make_volume_device(VOLUME, VOLUME, VOLUME)
        host = rng.random(VOLUME ** 3, dtype=np.float32).reshape(VOLUME, VOLUME, VOLUME)

        be.copy_h2d(B.Volume(host, VOLUME, VOLUME, VOLUME), v)
        found = []

        def collect():   # (the binarized volume holds 1.0 where a voxel was hit: every later call finds the same voxels)
            found.append(len(be.metal_collect(v, 1.0 - HIT_FRACTION, binarize=True)[0]))

        out["collect wall us, %d^3" % VOLUME] = timed_calls(be, collect, args.reps)
        assert len(set(found)) == 1
        out["collected"] = found[0]
        be.free(v)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
