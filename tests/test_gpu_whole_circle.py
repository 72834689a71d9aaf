"""The whole circle at full plane size, bit for bit against the CPU oracle ("What's weak" 2 and 3).

Every projection of BASELINE configs 3 and 2, and every 5th of config 5's 3600 (the 45 degree multiples included), goes through
the detector plane of that config into its full volume -- the angle-dependent choices of the backprojection (box orientation per
octant, the range of the shared-reciprocal division, the skip of tiles no ray reaches, the checked and global-tap fall-backs) and
the large-plane tile paths all run, at every angle. Three runs per case, each regenerating the raw frames one at a time from their
index (the stack is never held on the host):

  plain       one launch per call (what bench.py times): upload, weight, filter, read back, backproject. The oracle backprojects
              the frames READ BACK (config 5: the half frames, widened) into a few pairs of slices, on a worker thread while the
              GPU works, and those slices must equal the volume bit for bit. Sampled frames also check the weighting bit for bit,
              the filter row by row against a float64 FFT, and the half rounding.
  references  the product path (Backend.set_paris_loop_defaults(48), as paris::hip::set_device configures it) in PARIS's loop
              -- buffer per projection, upload, weight, filter, backproject, free -- on the raw frames.
  snapshots   the same with deferral by reference off and a depth of 37, which divides neither 1440 nor 720 (a partial last group).

Both product volumes must equal the plain one on EVERY voxel (int32 views on the device: the sign of each zero counts). A mismatch
reports per-slice counts, the first differing voxel, the largest difference and the runs of differing z, so that one run explains it.
"""
import collections
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

FILTER_TOL = 1e-5
SCALE = np.float32(40.0)   # raw frame i = (lcg(i) - 0.5) * SCALE
SAMPLED = 15               # frames per run that also check weight, filter and half rounding
CORNER = 64                # edge of the corner columns checked after the first projection

CASES = {
    # name: (detector n, projections of the circle, step between the indices used, grid edge, roi or None, half-precision frames,
    #        first z of each oracle slice pair: the volume's edges and tile boundaries; config 5's are relative to the ROI)
    "C3": (2048, 1440, 1, 2048, None, False, (0, 1023, 1337, 2046)),
    "C2": (1024, 720, 1, 1024, None, False, (0, 511, 1022)),
    "C5": (2048, 3600, 5, 4096, (1024, 3072, 1024, 3072, 1024, 3072), True, (0, 1023, 2046)),
}


def device_view(torch, v, dev):
    class _Mem:
        def __init__(self, ptr, shape):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Mem(v.ptr, (v.dim_z, v.dim_y, v.dim_x)), device=dev)


def raw_frame(oracle, n, i):
    f = oracle.lcg_projection(n, n, i)
    f -= np.float32(0.5)
    f *= SCALE
    return f


def frames_ahead(oracle, n, idxs, depth=3):
    """(position, index, raw frame) for every index, in order; the frames are made on worker threads a few ahead of the caller
    (the generator and numpy let go of the GIL), so at most depth + 1 of them are alive at once"""
    with ThreadPoolExecutor(2) as ex:
        ahead = collections.deque(ex.submit(raw_frame, oracle, n, i) for i in idxs[:depth])
        for j, i in enumerate(idxs):
            f = ahead.popleft().result()
            if j + depth < len(idxs):
                ahead.append(ex.submit(raw_frame, oracle, n, idxs[j + depth]))
            yield j, i, f


def upload(be, d_p, frame):
    """the frame through pinned memory of the ctx's pool onto the upload stream (PARIS's loop through paris::hip)"""
    h = C.c_void_p()
    _lib.check(be._L.paris_hip_malloc_host(be._ctx, frame.nbytes, C.byref(h)), "paris_hip_malloc_host")
    C.memmove(h.value, frame.ctypes.data, frame.nbytes)
    _lib.check(be._L.paris_hip_upload_projection(be._ctx, d_p.ptr, d_p.pitch, h.value, frame.shape[1] * 4, frame.shape[1],
                                                 frame.shape[0]), "paris_hip_upload_projection")
    _lib.check(be._L.paris_hip_free_host(be._ctx, h), "paris_hip_free_host")


def to_host(be, d_p):
    h = be.make_projection_host(d_p.dim_x, d_p.dim_y)
    be.copy_d2h(d_p, h)
    return h.buf


def half_to_host(be, ptr, pitch, n_x, n_y):
    out = np.empty((n_y, n_x), np.float16)
    _lib.check(be._L.paris_hip_memcpy_projection_d2h(be._ctx, out.ctypes.data, n_x * 2, ptr, pitch, n_x // 2, n_y),
               "paris_hip_memcpy_projection_d2h")
    be.synchronize()
    return out


def z_runs(zs):
    """[3, 4, 5, 9] -> '3-5, 9'"""
    runs, start = [], None
    for k, z in enumerate(zs):
        if start is None:
            start = z
        if k + 1 == len(zs) or zs[k + 1] != z + 1:
            runs.append("%d" % start if start == z else "%d-%d" % (start, z))
            start = None
    return ", ".join(runs)


def compare_slices(label, got, want, z0, problems):
    """host arrays of the same slices, z0 the first one's z: bit for bit, or a report in problems"""
    ne = got.view(np.uint32) != want.view(np.uint32)
    if not ne.any():
        return
    counts = ne.sum(axis=(1, 2))
    bad = [int(k) for k in np.flatnonzero(counts)]
    per_slice = ", ".join("z %d: %d" % (z0 + k, counts[k]) for k in bad[:8])
    if len(bad) > 8:
        per_slice += "; %d slices in all, z (runs) %s" % (len(bad), z_runs([z0 + k for k in bad]))
    z, y, x = (int(v) for v in np.argwhere(ne)[0])
    diff = np.abs(got[ne].astype(np.float64) - want[ne].astype(np.float64))
    problems.append("%s: differing voxels per slice (%s); first at (z, y, x) = (%d, %d, %d): %r, the oracle %r; largest |difference| %g"
                    % (label, per_slice, z0 + z, y, x, float(got[z, y, x]), float(want[z, y, x]), float(np.nanmax(diff))))


def compare_volumes(torch, label, got, want, problems, chunk=128):
    """two device volumes of the same shape on every voxel (int32 views), reduced on the device"""
    a, b = got.view(torch.int32), want.view(torch.int32)
    counts = torch.empty(a.shape[0], dtype=torch.int64, device=a.device)
    for z0 in range(0, a.shape[0], chunk):
        counts[z0:z0 + chunk] = (a[z0:z0 + chunk] != b[z0:z0 + chunk]).sum(dim=(1, 2))
    counts = counts.cpu().numpy()
    bad = [int(z) for z in np.flatnonzero(counts)]
    if not bad:
        return
    z = bad[0]
    y, x = (int(v) for v in torch.nonzero(a[z] != b[z])[0])
    largest = 0.0
    for z0 in sorted({zz // chunk * chunk for zz in bad}):
        ne = a[z0:z0 + chunk] != b[z0:z0 + chunk]
        d = (got[z0:z0 + chunk].double() - want[z0:z0 + chunk].double()).abs()
        largest = max(largest, float(torch.where(ne, d, torch.zeros_like(d)).max()))
        del ne, d
    worst = sorted(bad, key=lambda zz: -counts[zz])[:8]
    problems.append("%s: %d voxels in %d slices differ; z (runs): %s; most in z %s; first at (z, y, x) = (%d, %d, %d): %r, the plain "
                    "run %r; largest |difference| %g"
                    % (label, int(counts.sum()), len(bad), z_runs(bad), ", ".join("%d (%d)" % (zz, counts[zz]) for zz in worst),
                       z, y, x, float(got[z, y, x]), float(want[z, y, x]), largest))


def check_filter_rows(label, got, weighted, k64, fs, problems):
    """the filtered frame against irfft(rfft(weighted, fs) * K64)[:n] in float64, ROW BY ROW: relative L2 and max-abs relative to
    the row's own largest value"""
    n = weighted.shape[1]
    exact = np.fft.irfft(np.fft.rfft(weighted.astype(np.float64), fs, axis=1) * k64[None, :], fs, axis=1)[:, :n]
    err = got.astype(np.float64) - exact
    rel_l2 = np.sqrt((err ** 2).sum(axis=1) / np.maximum((exact ** 2).sum(axis=1), 1e-300))
    rel_max = np.abs(err).max(axis=1) / np.maximum(np.abs(exact).max(axis=1), 1e-300)
    rows = np.flatnonzero(~((rel_l2 <= FILTER_TOL) & (rel_max <= FILTER_TOL)))   # (a NaN fails too)
    if rows.size:
        problems.append("%s: %d detector rows filtered beyond %g of float64 (rows %s); worst relative L2 %g (row %d), worst max-abs %g "
                        "(row %d)" % (label, rows.size, FILTER_TOL, z_runs([int(r) for r in rows]), float(np.nanmax(rel_l2)),
                                      int(np.nanargmax(rel_l2)), float(np.nanmax(rel_max)), int(np.nanargmax(rel_max))))


@pytest.mark.parametrize("case", ["C2", "C3", "C5"])
def test_whole_circle_against_the_oracle(oracle, case):
    import torch
    n, n_circle, step, grid, roi_t, f16, pairs = CASES[case]
    g = (n, n, 0.2, 0.2, 0, 0, 500, 500, 360.0 / n_circle)
    det, odet = B.DetectorGeometry(*g), oracle.DetectorGeometry(*g)
    nat = B.calculate_volume_geometry(det)
    l_vx = float(np.float32(nat.l_vx_x) * np.float32(n) / np.float32(grid))
    vg, ovg = B.VolumeGeometry(grid, grid, grid, l_vx, l_vx, l_vx), oracle.VolumeGeometry(grid, grid, grid, l_vx, l_vx, l_vx)
    roi = B.RegionOfInterest(*roi_t) if roi_t else None
    oroi = oracle.RegionOfInterest(*roi_t) if roi_t else None
    out = B.apply_roi(vg, *roi_t) if roi_t else vg
    dx, dy, dz = out.dim_x, out.dim_y, out.dim_z
    assert dx == dy == dz == (1024 if case == "C2" else 2048)
    idxs = list(range(0, n_circle, step))
    assert len(idxs) == (1440 if case == "C3" else 720)
    if step > 1:
        assert all(i in idxs for i in range(0, n_circle, n_circle // 8))          # the 45 degree multiples
    vol_bytes = 4 * dx * dy * dz
    free, _ = torch.cuda.mem_get_info(0)
    if free < 2 * vol_bytes + (8 << 30):
        pytest.skip("needs %d GiB of free HBM" % ((2 * vol_bytes >> 30) + 8))
    dev = torch.device("cuda", 0)
    ds, dt = oracle.backproject_constants(odet, 0)[2:]   # detector offsets in mm, the same for every projection
    angles = {i: B.stage_angle(det, i) for i in idxs}
    sampled = set(int(j) for j in np.linspace(0, len(idxs) - 1, SAMPLED).round())
    fs = oracle.filter_size(n)
    k64 = odet.l_px_row * np.abs(np.fft.rfft(oracle.make_filter_real(fs, odet.l_px_row).astype(np.float64)))
    problems, timing = [], {}

    # ---- the oracle's slice pairs, fed by a worker thread in projection order ---------------------------------------------------
    want = [np.zeros((2, dy, dx), np.float32) for _ in pairs]
    oracle_s = [0.0]

    def oracle_add(frame, i):
        t0 = time.perf_counter()
        s, c, ods, odt = oracle.backproject_constants(odet, i)
        if (np.float32(s), np.float32(c)) != (np.float32(angles[i][0]), np.float32(angles[i][1])):
            problems.append("%s: projection %d: the library's angle (%r, %r) is not the oracle's (%r, %r)" % (case, i, *angles[i], s, c))
        for w, z in zip(want, pairs):
            oracle.backproject(w, frame, z, odet, ovg, s, c, ods, odt, oroi)   # v_offset = z (+ roi.z1 inside the oracle)
        oracle_s[0] += time.perf_counter() - t0

    # ---- plain run: one launch per call ---------------------------------------------------------------------------------------
    t_start = time.perf_counter()
    pbe = B.Backend(0, synchronous=False)
    try:
        pbe.set_backproject_deferral(1)
        pbe.set_stage_fusion(False)
        pbe.set_backproject_references(False)
        v_plain = pbe.make_volume_device(dx, dy, dz)
        t_plain = device_view(torch, v_plain, dev)
        with ThreadPoolExecutor(1) as worker:
            pending = collections.deque()
            for j, i, raw in frames_ahead(oracle, n, idxs):
                s, c = angles[i]
                d_p = pbe.make_projection_device(n, n)
                upload(pbe, d_p, raw)
                d_p.idx = i
                B.weight(pbe, d_p, det)
                if j in sampled:
                    weighted = to_host(pbe, d_p)
                    want_w = oracle.weight(raw.copy(), odet)
                    if not np.array_equal(weighted.view(np.uint32), want_w.view(np.uint32)):
                        problems.append("%s: projection %d: the weighted frame differs from the oracle in %d pixels"
                                        % (case, i, int((weighted.view(np.uint32) != want_w.view(np.uint32)).sum())))
                B.filter(pbe, d_p, det)
                filtered = to_host(pbe, d_p) if (j in sampled or not f16) else None
                if f16:
                    d16, p16 = pbe.convert_projection_f16(d_p)
                    half = half_to_host(pbe, d16, p16, n, n)
                    pbe.backproject_f16(d16, p16, n, n, v_plain, 0, det, vg, True, roi, s, c, ds, dt)
                    pbe.free(d16)
                    frame = half.astype(np.float32)
                else:
                    B.backproject(pbe, d_p, v_plain, 0, det, vg, False, False, None)
                    frame = filtered
                pbe.free(d_p)
                pending.append(worker.submit(oracle_add, frame, i))
                if j == 0:
                    # the first projection alone: the volume's corner columns against the oracle; on the full grids the corners on the
                    # source side are out of its rays -- tiles the launch skipped, still +0
                    pbe.synchronize()
                    torch.cuda.synchronize()
                    for y1, x1 in ((0, 0), (0, dx - CORNER), (dy - CORNER, 0), (dy - CORNER, dx - CORNER)):
                        got_c = t_plain[:, y1:y1 + CORNER, x1:x1 + CORNER].cpu().numpy()
                        r0 = roi_t if roi_t else (0, 0, 0, 0, 0, 0)
                        want_c = np.zeros((dz, CORNER, CORNER), np.float32)
                        oracle.backproject(want_c, frame, 0, odet, ovg, s, c, ds, dt,
                                           oracle.RegionOfInterest(r0[0] + x1, r0[0] + x1 + CORNER, r0[2] + y1, r0[2] + y1 + CORNER,
                                                                   r0[4], r0[4] + dz))
                        compare_slices("%s: projection %d alone, corner column at (y, x) = (%d, %d), positions within it" % (case, i, y1, x1), got_c, want_c,
                                       0, problems)
                        if roi_t is None and x1 == 0 and not (want_c.view(np.uint32) == 0).any():
                            problems.append("%s: the source-side corner column (%d, %d) is all in the rays of projection %d: the check "
                                            "saw no skipped tile" % (case, y1, x1, i))
                if j in sampled:
                    check_filter_rows("%s: projection %d" % (case, i), filtered, want_w.astype(np.float64), k64, fs, problems)
                    if f16 and not np.array_equal(half.view(np.uint16), filtered.astype(np.float16).view(np.uint16)):
                        problems.append("%s: projection %d: the half frame is not the filtered frame rounded to nearest even in %d "
                                        "pixels" % (case, i, int((half.view(np.uint16) != filtered.astype(np.float16).view(np.uint16)).sum())))
                while len(pending) > 2:
                    pending.popleft().result()
            while pending:
                pending.popleft().result()
        pbe.synchronize()
        torch.cuda.synchronize()
        timing["plain"] = time.perf_counter() - t_start
        updates = len(idxs) * len(pairs) * 2 * dx * dy
        timing["oracle GVox/s"] = updates / oracle_s[0] / 1e9

        for w, z in zip(want, pairs):
            compare_slices("%s: plain run against the oracle" % case, t_plain[z:z + 2].cpu().numpy(), w, z, problems)
            # something was compared: most of each slice lies in the field of view (config 5's ROI: all of it)
            for k in range(2):
                nonzero = int(np.count_nonzero(w[k]))
                if not (nonzero == dx * dy if roi_t else nonzero > 0.5 * dx * dy):
                    problems.append("%s: the oracle's slice z %d has only %d nonzero voxels of %d" % (case, z + k, nonzero, dx * dy))

        # ---- the product path, by reference and with snapshots -------------------------------------------------------------
        for name, depth, refs in (("references", 48, True), ("snapshots", 37, False)):
            t0 = time.perf_counter()
            with B.Backend(0, synchronous=False) as abe:
                abe.set_paris_loop_defaults(depth)
                abe.set_backproject_references(refs)
                v = abe.make_volume_device(dx, dy, dz)
                for j, i, raw in frames_ahead(oracle, n, idxs):
                    d_p = abe.make_projection_device(n, n)
                    upload(abe, d_p, raw)
                    d_p.idx = i
                    B.weight(abe, d_p, det)
                    B.filter(abe, d_p, det)
                    if f16:
                        s, c = angles[i]
                        d16, p16 = abe.convert_projection_f16(d_p)
                        abe.backproject_f16(d16, p16, n, n, v, 0, det, vg, True, roi, s, c, ds, dt)
                        abe.free(d16)
                    else:
                        B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
                    abe.free(d_p)
                abe.flush()
                abe.synchronize()
                torch.cuda.synchronize()
                timing[name] = time.perf_counter() - t0
                compare_volumes(torch, "%s: %s run (depth %d) against the plain run" % (case, name, depth), device_view(torch, v, dev),
                                t_plain, problems)
                torch.cuda.synchronize()
                abe.free(v)      # before the next volume: at most two of them live
        del t_plain
        pbe.free(v_plain)
    finally:
        pbe.close()
    timing["total"] = time.perf_counter() - t_start
    print("%s: %s" % (case, ", ".join("%s %.1f%s" % (k, v, "" if "/" in k else " s") for k, v in timing.items())))
    assert not problems, "\n".join(problems)
