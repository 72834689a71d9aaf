#!/usr/bin/env python3
"""Times paris_hip_detector_roll_rows on one GPU beside a device-to-device copy of the same bytes: one f32
frame of 2048 x 2048 and a group of 48, at eta = 0.5 and 5 degrees, and the roll search with 64 candidates on a mean of that size.
Every launch is bracketed by device events; a case is `reps` launches behind 5 warm-up launches, its figure their median.

  pass bytes  = 4 per pixel read + 4 per pixel written (the four taps of a pixel are shared with its neighbours through the caches)
  copy bytes  = the same
  ratio       = copy time / pass time
  margin      = the copy's own spread, (p90 - p10) / median of its launches, timed before and after the cases

  python tools/detector_roll_bench.py [--reps 20] [--frames 48] [--size 2048]
  python tools/detector_roll_bench.py --end-to-end DIR [--size 2048] [--views 120]   # paris.hip with and without --detector-roll
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
WARM = 5


def kernels(args):
    import torch

    from paris_amd import backend as B
    n = args.size
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    det = B.DetectorGeometry(n, n, 0.2, 0.2, 0.3, -0.2, 500, 500, 0.25)

    def timed(call):
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        pairs = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            pairs.append((a, b))
        be.synchronize()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)   # us

    out = {"frame": [n, n], "reps": args.reps}
    for frames in (1, args.frames):
        src = torch.rand((frames, n, n), dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        nbytes = 2 * 4 * frames * n * n
        first, d_first = be.wrap_projection(src.data_ptr(), 4 * n, n, n), be.wrap_projection(dst.data_ptr(), 4 * n, n, n)

        def copy_case():
            us = timed(lambda: dst.copy_(src))
            med = statistics.median(us)
            return {"median_us": round(med, 1), "min_us": round(us[0], 1), "p10_us": round(us[len(us) // 10], 1),
                    "p90_us": round(us[(9 * len(us)) // 10], 1), "bytes": nbytes, "TB_per_s": round(nbytes / med / 1e6, 3)}

        case = {"copy before": copy_case()}
        for eta in (0.5, 5.0):
            us = timed(lambda: be.detector_roll(first, d_first, src_frame_stride=4 * n * n if frames > 1 else 0,
                                                dst_frame_stride=4 * n * n if frames > 1 else 0, n_frames=frames, eta_deg=eta, det_geo=det))
            med = statistics.median(us)
            case["roll %g deg" % eta] = {"median_us": round(med, 1), "min_us": round(us[0], 1), "bytes": nbytes, "TB_per_s": round(nbytes / med / 1e6, 3)}
        case["copy after"] = copy_case()
        rate = (case["copy before"]["TB_per_s"] + case["copy after"]["TB_per_s"]) / 2
        case["copy_TB_per_s"] = round(rate, 3)
        case["margin"] = round(max([(c["p90_us"] - c["p10_us"]) / c["median_us"] for c in (case["copy before"], case["copy after"])]
                                   + [abs(case["copy before"]["TB_per_s"] - case["copy after"]["TB_per_s"]) / rate]), 4)
        for k, v in case.items():
            if k.startswith("roll "):
                v["of_copy_rate"] = round(v["TB_per_s"] / rate, 3)
        out["%d frame(s)" % frames] = case
        del src, dst
    # the search: the host clock around whole calls (upload of the mean, 64 rolls and scores, the totals, the copy back, the estimate)
    y, x = np.mgrid[:n, :n]
    mean = (np.exp(-((x - 0.55 * n) ** 2 + (y - 0.3 * n) ** 2) / (0.02 * n * n)) + np.exp(-((x - 0.3 * n) ** 2 + (y - 0.7 * n) ** 2) / (0.01 * n * n))).astype(np.float32)
    walls = []
    for _ in range(1 + 5):
        t0 = time.perf_counter()
        res, cost, pairs = be.find_detector_roll(mean, -3.15, 0.1, 64, det)
        walls.append(time.perf_counter() - t0)
    out["search, 64 candidates"] = {"wall_ms_first": round(walls[0] * 1e3, 2), "wall_ms_median_of_5": round(statistics.median(walls[1:]) * 1e3, 2),
                                    "pairs": int(pairs[0]), "margins": [res.margin_x, res.margin_y]}
    print(json.dumps(out, indent=1))
    be.close()


def end_to_end(args):
    from oracle import formats as F
    n, views = args.size, args.views
    root = args.end_to_end
    os.makedirs(os.path.join(root, "counts"), exist_ok=True)
    rng = np.random.default_rng(2)
    per_file = 20
    for k in range(0, views, per_file):
        m = min(per_file, views - k)
        fr = rng.integers(0, 40000, (m, n, n), dtype=np.uint16)
        open(os.path.join(root, "counts", "p%04d.his" % k), "wb").write(F.his_file_bytes(fr, 4))
    geo = os.path.join(root, "geo.ini")
    keys = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")
    open(geo, "w").write("\n".join("%s = %s" % kv for kv in zip(keys, (n, n, 0.2, 0.2, 0.0, 0.0, 500, 500, 360.0 / views))) + "\n")
    exe = os.path.join(ROOT, "paris_amd", "host", "demo", "paris.hip")
    out = {"detector": [n, n], "views": views, "runs": []}
    for rep in range(2):   # alternating
        for extra in ([], ["--detector-roll", "0.5"]):
            o = os.path.join(root, "out")
            t0 = time.time()
            # the central half of the volume's columns and 128 of its slices, so that the output stays small; --no-row-band: every frame
            # is still uploaded, rolled and filtered whole
            r = subprocess.run([exe, "--geometry", geo, "--input", os.path.join(root, "counts"), "--output", o, "--devices", "1", "--roi", "--roi-x1", str(n // 4),
                                "--roi-x2", str(3 * n // 4), "--roi-y1", str(n // 4), "--roi-y2", str(3 * n // 4), "--roi-z1", str(n // 2 - 64),
                                "--roi-z2", str(n // 2 + 64), "--no-row-band"] + extra, capture_output=True, text=True, timeout=900)
            wall = time.time() - t0
            if r.returncode != 0:
                raise SystemExit(r.stdout + r.stderr)
            line = [l for l in r.stdout.splitlines() if l.startswith("volume ")][0]
            out["runs"].append({"options": " ".join(extra) or "(none)", "process_wall_s": round(wall, 3), "report": line})
            for f in os.listdir(o):
                os.remove(os.path.join(o, f))
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--views", type=int, default=120)
    ap.add_argument("--end-to-end", metavar="DIR", help="write a synthetic scan under DIR and run paris.hip on it with and without --detector-roll 0.5")
    args = ap.parse_args()
    if args.end_to_end:
        return end_to_end(args)
    return kernels(args)


if __name__ == "__main__":
    main()
