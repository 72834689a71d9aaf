#!/usr/bin/env python3
"""Launches the dark / flat correction on one GPU, for a kernel trace: per 2048^2 u16 frame the widening alone (the raw upload
without a setting), the fused widening + correction (the corrected raw upload), and the in-place pass on an f32 frame, `reps` of
each. Prints the wall time per call from device events (uploads include their H2D copy); the kernel times come from the trace:

  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/flat_field_bench.py [--reps 200]

Bytes per pixel: widen 2 + 4, fused 2 + 4 + 8 (dark and flat), in place 4 + 4 + 8.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch

    from paris_amd import backend as B
    n = 2048
    rng = np.random.default_rng(1)
    dark = (200 + 100 * rng.random((n, n))).astype(np.float32)
    flat = (dark + 50000 * (0.8 + 0.2 * rng.random((n, n)))).astype(np.float32)
    frame = np.clip(dark + (flat - dark) * np.exp(-3 * rng.random((n, n))), 0, 65535).astype(np.uint16)
    dev = torch.device("cuda", 0)
    be = B.Backend(0, stream=torch.cuda.current_stream(dev).cuda_stream, synchronous=False)
    d = be.make_projection_device(n, n)
    be.set_flat_field(dark, flat)
    hv = np.ascontiguousarray(frame)
    out = {}
    cases = (("widen u16 (upload_raw)", lambda: be.upload_raw(hv, d), 6),
             ("widen + correct u16 (upload_raw corrected)", lambda: be.upload_raw(hv, d, corrected=True), 14),
             ("in place f32 (flat_field_rows)", lambda: be.flat_field_rows(d), 16))
    for name, call, bpp in cases:
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        be.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            call()
        b.record()
        be.synchronize()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / args.reps
        out[name] = {"us_per_call_wall": round(us, 3), "kernel_bytes": bpp * n * n}
    be.clear_flat_field()
    be.free(d)
    be.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
