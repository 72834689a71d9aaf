#!/usr/bin/env python3
"""Launches the forward projector (paris_hip_forward_project, forward_project.hip) on one GPU, for a kernel trace: one view per launch
of a 2048^2 detector over a 2048^3 volume, of a 1024^2 detector over a 1024^3 volume and of the 2048^2 detector over the central
2048 x 2048 x 256 slab, at 90 degrees (every ray y-marching: coalesced taps), 0 degrees (every ray x-marching: a line per lane) and 45
degrees (both), `reps` launches each after 10 warm-up launches. Prints the wall time per launch from device events; the kernel time
comes from the trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/forward_project_bench.py [--reps 200] [--cases 1024,slab,2048]
  python tools/forward_project_bench.py --summarise <dir> [--reps 200] [--cases ...]   # medians per case and angle from the trace

and for counters, in a run of their own (a few launches are enough):

  rocprofv3 --pmc <counters> --output-format csv -d <dir> -- python tools/forward_project_bench.py --reps 3 --warmup 1 --cases 1024
  python tools/forward_project_bench.py --counters <dir> --reps 3 --warmup 1 --cases 1024

The launches of the trace are told apart by their order: --summarise and --counters need the --reps, --warmup and --cases of the run.
Floor: the volume read once, 4 bytes per voxel per view.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ANGLES = (("90 deg (y-marching)", 90.0), ("0 deg (x-marching)", 0.0), ("45 deg (both)", 45.0))
# name -> (detector and grid width n, slab depth, slab offset)
CASES = {"2048": (2048, 2048, 0), "1024": (1024, 1024, 0), "slab": (2048, 256, 896)}
KERNEL = "forward_project_kernel"


def schedule(args):
    """(case, angle name, angle, launches) in launch order"""
    return [(c, name, a, args.warmup + args.reps) for c in args.cases for name, a in ANGLES]


def run(args):
    import math

    import numpy as np
    import torch

    from paris_amd import backend as B
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    out = {}
    for case in args.cases:
        n, depth, offset = CASES[case]
        det = B.DetectorGeometry(n, n, 0.2, 0.2, 0.0, 0.0, 500, 500, 1.0)
        vg = B.VolumeGeometry(n, n, n, 0.1, 0.1, 0.1)
        vol = torch.rand((depth, n, n), dtype=torch.float32, device=dev)
        d_v = be.wrap_volume(vol.data_ptr(), n, n, depth, owner=vol)
        d_p = be.make_projection_device(n, n)
        for name, angle in ANGLES:
            a = np.float32(angle) * (np.float32(math.pi) / np.float32(180.0))
            s, c = float(np.float32(math.sin(a))), float(np.float32(math.cos(a)))
            for _ in range(args.warmup):
                be.forward_project(d_v, offset, det, vg, d_p, s, c, 0.0, 0.0)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.reps):
                be.forward_project(d_v, offset, det, vg, d_p, s, c, 0.0, 0.0)
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / args.reps
            out["%s, %s" % (case, name)] = {"us_per_launch_wall": round(us, 1), "volume_bytes": 4 * n * n * depth,
                                            "GB_per_s_wall": round(4 * n * n * depth / us / 1e3, 1)}
        be.free(d_p)
        del vol
        torch.cuda.empty_cache()
    be.close()
    print(json.dumps(out))


def trace_rows(directory, pattern):
    rows = []
    for f in glob.glob(directory + "/**/*" + pattern, recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if KERNEL in r["Kernel_Name"]]
    return rows


def summarise(args):
    rows = sorted(trace_rows(args.summarise, "_kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    plan = schedule(args)
    if len(rows) != sum(p[3] for p in plan):
        raise SystemExit("the trace holds %d launches of %s, the schedule %d: pass the run's --reps, --warmup and --cases"
                         % (len(rows), KERNEL, sum(p[3] for p in plan)))
    out, at = {}, 0
    for case, name, _, count in plan:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[at + args.warmup:at + count]]
        r0 = rows[at]
        at += count
        n, depth, _ = CASES[case]
        med = statistics.median(us)
        out["%s, %s" % (case, name)] = {"launches": len(us), "us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                                        "volume_bytes": 4 * n * n * depth, "TB_per_s_of_the_floor": round(4 * n * n * depth / med / 1e6, 3),
                                        "GVoxel_samples_per_s": round(n * n * depth / med / 1e3, 1),
                                        "vgpr": r0.get("VGPR_Count") or r0.get("Arch_VGPR_Count"), "scratch": r0.get("Scratch_Size") or r0.get("Private_Segment_Size"),
                                        "grid": [r0.get("Grid_Size_X"), r0.get("Grid_Size_Y"), r0.get("Grid_Size_Z")]}
    print(json.dumps(out, indent=1))


def counters(args):
    rows = trace_rows(args.counters, "_counter_collection.csv")
    ids = sorted({int(r["Dispatch_Id"]) for r in rows})
    plan = schedule(args)
    if len(ids) != sum(p[3] for p in plan):
        raise SystemExit("the run holds %d launches of %s, the schedule %d: pass the run's --reps, --warmup and --cases"
                         % (len(ids), KERNEL, sum(p[3] for p in plan)))
    out, at = {}, 0
    for case, name, _, count in plan:
        mine = set(ids[at + args.warmup:at + count])
        at += count
        acc = {}
        for r in rows:
            if int(r["Dispatch_Id"]) in mine:
                acc.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
        out["%s, %s" % (case, name)] = {k: sum(v) / len(v) for k, v in sorted(acc.items())}
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="1024,slab,2048", help="comma-separated, of " + ", ".join(CASES))
    ap.add_argument("--summarise", metavar="DIR", help="medians from the kernel trace under DIR instead of a run")
    ap.add_argument("--counters", metavar="DIR", help="mean counter values per case and angle from the --pmc run under DIR")
    args = ap.parse_args()
    args.cases = [c for c in args.cases.split(",") if c]
    for c in args.cases:
        if c not in CASES:
            raise SystemExit("unknown case %s" % c)
    if args.summarise:
        summarise(args)
    elif args.counters:
        counters(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
