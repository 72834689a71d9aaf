#!/usr/bin/env python3
"""Times paris_hip_bin_frames on one GPU beside a device-to-device copy of the same source bytes:
48 f32 frames of 4096 x 4096, one under the other, binned 2 x 2 and 4 x 4, with and without a mask (3 % of the pixels bad).
Every launch is bracketed by device events; a case is `reps` launches behind 5 warm-up launches, its figure their median.

  pass bytes  = 4 per source pixel read + 1 per source pixel with a mask + 4 per binned pixel written
  copy bytes  = 4 per source pixel read + 4 written
  ratio       = (pass bytes / pass time) / (copy bytes / copy time)
  margin      = the copy's own spread, (p90 - p10) / median of its launches, timed before and after the cases

  python tools/binning_bench.py [--reps 20] [--frames 48] [--size 4096]
  python tools/binning_bench.py --end-to-end DIR [--size 1024] [--views 360]   # paris.hip with and without --bin 2 on a synthetic scan
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
    n, frames = args.size, args.frames
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    src = torch.rand((frames, n, n), dtype=torch.float32, device=dev) * 60000.0
    other = torch.empty_like(src)
    mask = (np.random.default_rng(1).random((n, n)) < 0.03).astype(np.uint8)
    first = be.wrap_projection(src.data_ptr(), 4 * n, n, n)
    src_bytes = 4 * frames * n * n

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

    def copy_case():
        us = timed(lambda: other.copy_(src))
        med = statistics.median(us)
        return {"median_us": round(med, 1), "min_us": round(us[0], 1), "p10_us": round(us[len(us) // 10], 1),
                "p90_us": round(us[(9 * len(us)) // 10], 1), "bytes": 2 * src_bytes, "TB_per_s": round(2 * src_bytes / med / 1e6, 3)}

    out = {"frames": frames, "frame": [n, n], "reps": args.reps, "copy before": copy_case()}
    for b in (2, 4):
        for masked in (False, True):
            be.set_binning(b, b, n, n, mask if masked else None)
            dst = torch.empty((frames, n // b, n // b), dtype=torch.float32, device=dev)
            d_first = be.wrap_projection(dst.data_ptr(), 4 * (n // b), n // b, n // b)
            us = timed(lambda: be.bin_frames(first, d_first, src_frame_stride=4 * n * n, dst_frame_stride=4 * (n // b) ** 2, n_frames=frames))
            med = statistics.median(us)
            nbytes = src_bytes + (frames * n * n if masked else 0) + src_bytes // (b * b)
            out["bin %d x %d%s" % (b, b, ", mask" if masked else "")] = {
                "median_us": round(med, 1), "min_us": round(us[0], 1), "bytes": nbytes, "TB_per_s": round(nbytes / med / 1e6, 3)}
            be.clear_binning()
            del dst
    out["copy after"] = copy_case()
    copy_rate = (out["copy before"]["TB_per_s"] + out["copy after"]["TB_per_s"]) / 2
    spreads = [(c["p90_us"] - c["p10_us"]) / c["median_us"] for c in (out["copy before"], out["copy after"])]
    out["copy_TB_per_s"] = round(copy_rate, 3)
    out["margin"] = round(max(spreads + [abs(out["copy before"]["TB_per_s"] - out["copy after"]["TB_per_s"]) / copy_rate]), 4)
    for k, v in out.items():
        if k.startswith("bin "):
            v["of_copy_rate"] = round(v["TB_per_s"] / copy_rate, 3)
    print(json.dumps(out, indent=1))
    be.close()


def end_to_end(args):
    from oracle import formats as F
    n, views = args.size, args.views
    root = args.end_to_end
    os.makedirs(os.path.join(root, "counts"), exist_ok=True)
    rng = np.random.default_rng(2)
    dark = rng.integers(150, 450, (1, n, n)).astype(np.uint16)
    flat = rng.integers(30000, 60000, (1, n, n)).astype(np.uint16)
    open(os.path.join(root, "dark.his"), "wb").write(F.his_file_bytes(dark, 4))
    open(os.path.join(root, "flat.his"), "wb").write(F.his_file_bytes(flat, 4))
    per_file = 40
    for k in range(0, views, per_file):
        m = min(per_file, views - k)
        t = np.exp(-3 * rng.random((m, n, n), dtype=np.float32))
        fr = np.clip(dark[0] + (flat[0].astype(np.float32) - dark[0]) * t, 0, 65535).astype(np.uint16)
        open(os.path.join(root, "counts", "p%04d.his" % k), "wb").write(F.his_file_bytes(fr, 4))
    geo = os.path.join(root, "geo.ini")
    keys = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")
    open(geo, "w").write("\n".join("%s = %s" % kv for kv in zip(keys, (n, n, 0.2, 0.2, 0.0, 0.0, 500, 500, 360.0 / views))) + "\n")
    exe = os.path.join(ROOT, "paris_amd", "host", "demo", "paris.hip")
    out = {"detector": [n, n], "views": views, "runs": []}
    for rep in range(2):   # alternating
        for extra in ([], ["--bin", "2"]):
            o = os.path.join(root, "out")
            t0 = time.time()
            r = subprocess.run([exe, "--geometry", geo, "--input", os.path.join(root, "counts"), "--output", o, "--flat", os.path.join(root, "flat.his"),
                                "--dark", os.path.join(root, "dark.his"), "--devices", "1"] + extra, capture_output=True, text=True, timeout=900)
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
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--views", type=int, default=360)
    ap.add_argument("--end-to-end", metavar="DIR", help="write a synthetic scan under DIR and run paris.hip on it with and without --bin 2")
    args = ap.parse_args()
    if args.end_to_end:
        args.size = args.size or 1024
        return end_to_end(args)
    args.size = args.size or 4096
    return kernels(args)


if __name__ == "__main__":
    main()
