#!/usr/bin/env python3
"""Launches the kernels of the starvation filter on one GPU, for a kernel trace:

  starvation_filter_kernel   paris_hip_starvation_filter_frames with R = 3 on 1 and on 16 frames of 2048^2 f32 line integrals (pitch 8192)
  starvation_store_kernel    with NO pixel above p0 -- both kernels read every pixel once and nothing else -- and with two discs per
                             frame, about 5 % of the pixels, above p0 at every level
  zinger_detect_kernel       paris_hip_zinger_filter_rows on the frames without discs: the yardstick (with zinger_apply_kernel)

The pass is not idempotent, so the frames are uploaded again before every call; only the kernels' times mean anything here, and they
come from the trace. `reps` timed calls each behind 3 warm-up calls, every configuration in a sequence of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/starvation_bench.py [--reps 10]
  python tools/starvation_bench.py --summarise <dir> [--reps 10]
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
FRAMES = (1, 16)
WARM = 3
P0 = 3.0
RADIUS = 3
LAUNCH_FRAMES = 8      # PARIS_HIP_STARVATION_FRAMES_MAX: 16 frames are two launches of each kernel


def frames_for():
    """(a smooth frame below p0 everywhere, the same with two discs of radius 185 pixels -- 2 pi 185^2 / 2048^2 = 5.1 % -- that rise
    from p0 to p0 + 4.5 towards their centres, with noise that grows with the level; the share of its pixels above p0)"""
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:N, 0:N]
    calm = (0.45 + 0.4 * np.sin(x / 97.0) * np.cos(y / 131.0)).astype(np.float32)
    starved = calm.copy()
    for cx, cy in ((700, 900), (1400, 1100)):
        r2 = ((x - cx) ** 2 + (y - cy) ** 2) / 185.0 ** 2
        inside = r2 < 1.0
        level = 4.5 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0))
        noise = rng.normal(0.0, 1.0, (N, N)) * 0.02 * np.exp(level / 2)
        starved[inside] = (P0 + 0.01 + level + np.abs(noise))[inside].astype(np.float32)
    return calm, starved, float((starved > np.float32(P0)).mean())


def summarise(directory, reps):
    rows = []
    for f in glob.glob(directory + "/**/*_kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}

    def medians(kernel, names, launches):
        """names[k] is a configuration of launches[k] launches per call: the median over the timed calls of a call's summed launches"""
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        if len(us) != (WARM + reps) * sum(launches):
            raise SystemExit("%s: %d launches in the trace, %d expected (give the run's --reps)" % (kernel, len(us), (WARM + reps) * sum(launches)))
        at = 0
        for name, per_call in zip(names, launches):
            calls = [sum(us[at + c * per_call:at + (c + 1) * per_call]) for c in range(WARM + reps)]
            at += (WARM + reps) * per_call
            timed = sorted(calls[WARM:])
            out["%s, %s" % (kernel, name)] = {"median_us": round(statistics.median(timed), 3), "min_us": round(timed[0], 3)}

    frames = ["%d frame(s)" % f for f in FRAMES]
    launches = [(f + LAUNCH_FRAMES - 1) // LAUNCH_FRAMES for f in FRAMES]
    for k in ("starvation_filter_kernel", "starvation_store_kernel"):
        medians(k, ["nothing above p0, " + f for f in frames] + ["5 % above p0, " + f for f in frames], launches * 2)
    medians("zinger_detect_kernel", frames, [1, 1])
    medians("zinger_apply_kernel", frames, [1, 1])
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--summarise")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.reps)
    from paris_amd import backend as B
    out = {}
    calm, starved, share = frames_for()
    out["share_above_p0"] = round(share, 4)
    with B.Backend(0, synchronous=False) as be:
        slots = be.make_projection_device(N, N * max(FRAMES))
        assert slots.pitch == 4 * N
        first = be.wrap_projection(slots.ptr, slots.pitch, N, N)
        stride = slots.pitch * N

        def upload(frame, n):
            for k in range(n):
                be.upload_raw(frame, be.wrap_projection(slots.ptr + k * stride, slots.pitch, N, N))

        be.set_starvation_filter((P0, 1.0, RADIUS), N, N)
        for label, frame in (("nothing above p0", calm), ("5 % above p0", starved)):
            for f in FRAMES:
                be.starvation_stats(reset=True)
                for _ in range(WARM + args.reps):
                    upload(frame, f)
                    be.starvation_filter(first, frame_stride=stride, n_frames=f)
                c = be.starvation_stats()
                out["%s, %d frame(s)" % (label, f)] = {"frames": c.frames, "filtered_per_frame": c.filtered / c.frames,
                                                       "last_level_per_frame": c.last_level / c.frames}
        be.clear_starvation_filter()
        be.set_zinger_filter(0.25, 0.0, 0, N, N)
        upload(calm, max(FRAMES))
        for f in FRAMES:
            for _ in range(WARM + args.reps):
                be.zinger_filter_rows(first, frame_stride=stride, n_frames=f)
        be.synchronize()
        be.clear_zinger_filter()
        be.free(slots)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
