#!/usr/bin/env python3
"""Launches the offset-detector redundancy weight (paris_hip_offset_detector_weight_rows) on one GPU, for a kernel trace: a whole
2048^2 frame at delta_s = -700 (an overlap of 324 pixels) and a 1024-row band of it, `reps` launches each. Prints the wall time per
launch from device events; the kernel time comes from the trace:

  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/offset_detector_bench.py [--reps 200]

Bytes per pixel: 8 (one read, one write).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch

    from paris_amd import backend as B
    n = 2048
    det = B.DetectorGeometry(n, n, 0.2, 0.2, -700.0, 0.0, 500, 500, 0.25)
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    d = be.make_projection_device(n, n)
    out = {}
    for name, r0, rows in (("frame 2048x2048", 0, n), ("band 1024 rows x 2048", 512, 1024)):
        for _ in range(10):
            be.offset_detector_weight(d, det, r0, rows)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            be.offset_detector_weight(d, det, r0, rows)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / args.reps
        out[name] = {"us_per_launch_wall": round(us, 3), "bytes": 8 * n * rows, "GB_per_s_wall": round(8 * n * rows / us / 1e3, 1)}
    be.free(d)
    be.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
