#!/usr/bin/env python3
"""Times the fused cosine weight + row filter (paris_hip_weight_filter_rows / _batch) with the row extension off and on: one n x n
frame per launch and a group of `--group` frames per launch, by device events. Talks to the library through ctypes alone, so
`--library` may name ANY build of the C ABI -- an older one without the row extension is timed with the setting off only (for an
A/B of library builds, run the tool once per build, alternately, in one session).

  python tools/row_extension_bench.py [--library path/to/libparis_hip.so] [--n 2048] [--group 48] [--reps 200] [--repeats 7]
                                      [--taper 16] [--edge 4]

One JSON line per (library, case): the median over the repeats of the mean time per launch (per frame for the group), and the
repeats' minimum and maximum -- the run-to-run spread. Run it alone under `rocprofv3 --kernel-trace --stats` for kernel times
(then with --repeats 1: the trace needs no repeats)."""
import argparse
import ctypes as C
import json
import os
import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RowExtension(C.Structure):
    _fields_ = [("edge_pixels", C.c_uint32), ("taper_pixels", C.c_uint32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=os.path.join(ROOT, "paris_amd", "lib", "libparis_hip.so"))
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--group", type=int, default=48)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--taper", type=int, default=16)
    ap.add_argument("--edge", type=int, default=4)
    args = ap.parse_args()
    import torch   # loaded first: the libraries bind to the HIP runtime torch ships

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    n, group = args.n, args.group
    tau = 0.2
    fsize = 2 << (n - 1).bit_length()
    consts = [C.c_float(v) for v in (-n * tau / 2, -n * tau / 2, 1000.0, tau, tau)]   # h_min, v_min, d_sd, l_px_row, l_px_col
    one = torch.rand((8, n, n), device=dev, dtype=torch.float32)
    stack = torch.rand((group, n, n), device=dev, dtype=torch.float32)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t

    path = args.library
    L = C.CDLL(path)
    ctx, k = vp(), vp()
    L.paris_hip_ctx_create.argtypes = [C.c_int, vp, C.c_uint, C.POINTER(vp)]
    assert L.paris_hip_ctx_create(0, vp(stream.cuda_stream), 0, C.byref(ctx)) == 0
    L.paris_hip_make_filter.argtypes = [vp, u32, C.c_float, C.POINTER(vp)]
    assert L.paris_hip_make_filter(ctx, fsize, tau, C.byref(k)) == 0
    L.paris_hip_weight_filter_rows.argtypes = [vp, vp, sz, u32, u32, u32, u32] + [C.c_float] * 5 + [vp, u32, vp, sz]
    L.paris_hip_weight_filter_batch.argtypes = [vp, vp, sz, sz, u32, u32, u32, u32, u32] + [C.c_float] * 5 + [vp, u32, vp, sz, sz]
    has = hasattr(L, "paris_hip_set_row_extension")   # an older build: timed with the setting off only
    if has:
        L.paris_hip_set_row_extension.argtypes = [vp, C.POINTER(RowExtension)]
        L.paris_hip_clear_row_extension.argtypes = [vp]

    def timed(body):
        for i in range(10):
            body(i)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.reps):
            body(i)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.reps * 1e3   # us

    def frame(i):
        assert L.paris_hip_weight_filter_rows(ctx, vp(one[i % 8].data_ptr()), n * 4, n, n, 0, n, *consts, k, fsize, None, 0) == 0

    def frames(i):
        assert L.paris_hip_weight_filter_batch(ctx, vp(stack.data_ptr()), n * 4, n * n * 4, group, n, n, 0, n, *consts, k, fsize, None, 0, 0) == 0

    results = {}
    for rep in range(args.repeats):
        for on in ((False, True) if has else (False,)):
            if has:
                setting = RowExtension(args.edge, args.taper)
                assert (L.paris_hip_set_row_extension(ctx, C.byref(setting)) if on else L.paris_hip_clear_row_extension(ctx)) == 0
            results.setdefault((on, "one_frame_us"), []).append(timed(frame))
            results.setdefault((on, "group_us_per_frame"), []).append(timed(frames) / group)
    for (on, case), v in results.items():
        print(json.dumps({"library": os.path.relpath(path, ROOT), "row_extension": on, "case": case, "detector": "%dx%d" % (n, n),
                          "filter_length": fsize, "group": group, "median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3),
                          "max_us": round(max(v), 3), "repeats": len(v), "reps": args.reps}), flush=True)
    L.paris_hip_free.argtypes = [vp, vp]
    L.paris_hip_free(ctx, k)
    L.paris_hip_ctx_destroy.argtypes = [vp]
    L.paris_hip_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
