#!/usr/bin/env python3
"""Times the axis search on one GPU: scoring `count` candidates on an N x n sinogram, collecting the band of
2048 x 2048 frames, the numpy rule on the CPU for scale, and the driver's pre-pass on a synthetic scan.

  python tools/axis_search_bench.py [--reps 10] [--views 1440] [--columns 2048] [--count 129]
      score:   paris_hip_axis_search_finish between two host clock readings with the ctx stream idle before: the score kernel, the
               per-candidate totals, a copy of 24 bytes per candidate and the stream wait. The search is opened and filled anew for
               every repetition (finish closes it); 2 warm-up repetitions, the figure is the median of the rest.
      collect: paris_hip_axis_search_add_rows of 64 frames of `columns` x `columns` float pixels (R = 2 rows each), timed the same way.
  python tools/axis_search_bench.py --rule [--processes 16]      # the numpy rule (tests/axis_rule.py), candidates dealt to processes
  python tools/axis_search_bench.py --end-to-end DIR [--size 1024] [--scan-views 360] [--other-exe PATH]
      paris.hip on a synthetic scan of u16 counts: --find-axis --axis-only, the same with --rings, and a reconstruction with --rings
      alone (its ring pre-pass time), the last also with another build's paris.hip (the parent commit's) when given
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GEO = dict(l_px_row=0.2, d_so=500.0, d_od=500.0)


def sinogram(views, columns):
    import axis_rule as A
    k = (columns * GEO["l_px_row"] / 4.0) / 34.56   # the discs of the 96-column case (half field of view 34.56 mm) scaled to this detector's
    discs = tuple((cx * k, cy * k, r * k, rho) for cx, cy, r, rho in A.DISCS)
    return A.disc_sinogram(views, columns, 2.4, discs, **GEO).astype(np.float32)


def kernels(args):
    from paris_amd import backend as B
    n_frames, n, count = args.views, args.columns, args.count
    lo, step = -0.125 * (count // 2), 0.125
    sino = sinogram(n_frames, n)
    det = B.DetectorGeometry(n, 1, GEO["l_px_row"], GEO["l_px_row"], 0.0, 0.0, GEO["d_so"], GEO["d_od"], 360.0 / n_frames)
    out = {"views": n_frames, "columns": n, "candidates": count, "pairs": count * n_frames * n}
    with B.Backend(0, synchronous=False) as be:
        d = be.make_projection_device(n, n_frames)
        be.upload_raw(sino, d)
        first = be.wrap_projection(d.ptr, d.pitch, n, 1)
        ms, begin_ms = [], []
        for rep in range(args.reps + 2):
            t0 = time.perf_counter()
            be.axis_search_begin(lo, step, count, det, n_frames, rows=1)
            begin_ms.append((time.perf_counter() - t0) * 1e3)
            be.axis_search_add(first, 0, frame_stride=d.pitch, n_frames=n_frames)
            be.synchronize()
            t0 = time.perf_counter()
            res, cost, columns = be.axis_search_finish()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms, begin_ms = sorted(ms[2:]), sorted(begin_ms[2:])
        out["score"] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
                        "gpairs_per_s": round(out["pairs"] / statistics.median(ms) / 1e6, 1), "estimate": float(res.delta_s),
                        "j_min_over_median": res.cost_min / res.cost_median, "begin_median_ms": round(statistics.median(begin_ms), 3)}
        be.free(d)
        frames, size = 64, n
        big = be.make_projection_device(size, size * frames)
        be.upload_raw(np.random.default_rng(1).random((size * frames, size), dtype=np.float32), big)
        det2 = B.DetectorGeometry(size, size, 0.2, 0.2, 0.0, 0.0, 500.0, 500.0, 360.0 / frames)
        p = be.wrap_projection(big.ptr, big.pitch, size, size)
        us = []
        for rep in range(args.reps + 2):
            be.axis_search_begin(-1.0, 1.0, 3, det2, frames, rows=2)
            be.synchronize()
            t0 = time.perf_counter()
            be.axis_search_add(p, 0, frame_stride=big.pitch * size, n_frames=frames)
            be.synchronize()
            us.append((time.perf_counter() - t0) * 1e6)
            be.axis_search_discard()
        us = sorted(us[2:])
        out["collect"] = {"frames": frames, "frame": [size, size], "rows": 2, "median_us": round(statistics.median(us), 1), "min_us": round(us[0], 1),
                          "band_bytes": frames * 2 * size * 4}
    print(json.dumps(out, indent=1))


def _rule_part(job):
    import axis_rule as A
    sino, lo, step, k0, k1, n_frames = job
    c = A.candidates(lo, step, k1)
    return [float(A.costs(sino, c[k], step, 1, n_frames, GEO["l_px_row"], GEO["d_so"], GEO["d_od"])[0][0]) for k in range(k0, k1)]


def rule(args):
    import multiprocessing as mp

    import axis_rule as A
    n_frames, n, count = args.views, args.columns, args.count
    lo, step = -0.125 * (count // 2), 0.125
    sino = sinogram(n_frames, n)
    edges = np.linspace(0, count, args.processes + 1).astype(int)
    jobs = [(sino, lo, step, int(a), int(b), n_frames) for a, b in zip(edges[:-1], edges[1:]) if b > a]
    t0 = time.perf_counter()
    with mp.Pool(args.processes) as pool:
        cost = sum(pool.map(_rule_part, jobs), [])
    wall = time.perf_counter() - t0
    est = A.estimate(lo, step, cost)
    print(json.dumps({"views": n_frames, "columns": n, "candidates": count, "processes": args.processes, "wall_s": round(wall, 2),
                      "estimate": float(est["delta_s"])}, indent=1))


def end_to_end(args):
    from oracle import formats as F
    n, views = args.size, args.scan_views
    root = args.end_to_end
    os.makedirs(os.path.join(root, "counts"), exist_ok=True)
    rng = np.random.default_rng(2)
    dark = rng.integers(150, 450, (1, n, n)).astype(np.uint16)
    flat = rng.integers(30000, 60000, (1, n, n)).astype(np.uint16)
    open(os.path.join(root, "dark.his"), "wb").write(F.his_file_bytes(dark, 4))
    open(os.path.join(root, "flat.his"), "wb").write(F.his_file_bytes(flat, 4))
    line = sinogram(views, n)
    line *= 3.0 / line.max()
    per_file = 40
    for k in range(0, views, per_file):
        m = min(per_file, views - k)
        t = np.exp(-np.repeat(line[k:k + m, None, :], n, axis=1)) * (1.0 + 0.01 * rng.standard_normal((m, n, n), dtype=np.float32))
        fr = np.clip(dark[0] + (flat[0].astype(np.float32) - dark[0]) * t, 0, 65535).astype(np.uint16)
        open(os.path.join(root, "counts", "p%04d.his" % k), "wb").write(F.his_file_bytes(fr, 4))
    geo = os.path.join(root, "geo.ini")
    keys = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")
    open(geo, "w").write("\n".join("%s = %s" % kv for kv in zip(keys, (n, n, 0.2, 0.2, 0.0, 0.0, 500, 500, 360.0 / views))) + "\n")
    exe = os.path.join(ROOT, "paris_amd", "host", "demo", "paris.hip")
    base = ["--geometry", geo, "--input", os.path.join(root, "counts"), "--output", os.path.join(root, "out"), "--flat", os.path.join(root, "flat.his"),
            "--dark", os.path.join(root, "dark.his"), "--devices", "1"]
    axis = ["--find-axis", "-8:8:0.125", "--axis-only"]
    cases = [("this tree", exe, axis), ("this tree", exe, axis + ["--rings", "2:0.05"]), ("this tree", exe, ["--rings", "2:0.05"])]
    if args.other_exe:
        cases.append(("other build", args.other_exe, ["--rings", "2:0.05"]))
    out = {"detector": [n, n], "views": views, "runs": []}
    for rep in range(2):   # alternating
        for who, program, extra in cases:
            t0 = time.time()
            r = subprocess.run([program] + base + extra, capture_output=True, text=True, timeout=900)
            wall = time.time() - t0
            if r.returncode != 0:
                raise SystemExit(r.stdout + r.stderr)
            lines = [l for l in r.stdout.splitlines() if l.startswith(("axis search on", "ring filter on", "volume ", "warning"))]
            out["runs"].append({"build": who, "options": " ".join(extra), "process_wall_s": round(wall, 3), "report": lines})
            o = os.path.join(root, "out")
            for f in os.listdir(o) if os.path.isdir(o) else []:
                os.remove(os.path.join(o, f))
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--views", type=int, default=1440)
    ap.add_argument("--columns", type=int, default=2048)
    ap.add_argument("--count", type=int, default=129)
    ap.add_argument("--rule", action="store_true", help="time the numpy rule on the CPU instead")
    ap.add_argument("--processes", type=int, default=16)
    ap.add_argument("--end-to-end", metavar="DIR", help="write a synthetic scan under DIR and run paris.hip's pre-pass on it")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--scan-views", type=int, default=360)
    ap.add_argument("--other-exe", help="another build's paris.hip for the ring pre-pass alone")
    args = ap.parse_args()
    if args.end_to_end:
        return end_to_end(args)
    return rule(args) if args.rule else kernels(args)


if __name__ == "__main__":
    main()
