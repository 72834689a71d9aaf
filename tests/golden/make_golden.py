"""Regenerates the golden fixtures in this directory from the CPU oracle (oracle/), which is itself pinned to
the reference by tests/test_oracle_kat.py. Run from the repo root:  python tests/golden/make_golden.py

Fixtures are data only (inputs are regenerated from the LCG; expected outputs are stored):
  kat.npz     KAT geometry of SURVEY.md 8c: weighted projection 0, the 8 filtered projections, the full
              67x67x61 volume, the ramp filter K for N in {128, 1024, 2048, 4096}
  cube64.npz  64^3 / 8 projections: three central slices, sum and abs-sum
  mkl_fft.npz MKL's FFTW transforms (libmkl_rt.so) of the KAT geometry's filter and 8 weighted projections, keyed by the
              sha256 of their inputs (tests/mkl_fftw.py: Recorded); written only where libmkl_rt.so exists
  fdk_model_bounds.json  the oracle's own error against the float64 model of tests/fdk_model.py on the cases of
              tests/fdk_cases.py, per case and stage (CPU only; alone:  python tests/golden/make_golden.py fdk_model_bounds)
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import oracle as O  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import mkl_fftw  # noqa: E402


def main():
    det = O.DetectorGeometry(64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 45)
    vg = O.calculate_volume_geometry(det)
    p0 = O.lcg_projection(64, 48, 0)
    O.weight(p0, det)
    filtered = []
    vol = O.reconstruct(det, vg, 8, filtered_out=filtered)
    ks = {"k_%d" % n: O.make_filter(n, 0.2) for n in (128, 1024, 2048, 4096)}
    np.savez_compressed(os.path.join(HERE, "kat.npz"), weighted_p0=p0, filtered=np.stack(filtered), volume=vol, **ks)

    d = O.DetectorGeometry(64, 64, 0.2, 0.2, 0, 0, 100, 200, 45.0)
    g = O.calculate_volume_geometry(d)
    v = O.reconstruct(d, g, 8)
    np.savez_compressed(os.path.join(HERE, "cube64.npz"), slices=v[31:34].copy(),
                        sum=np.float64(v.sum(dtype=np.float64)), abssum=np.float64(np.abs(v).sum(dtype=np.float64)))
    record_fdk_model_bounds()
    files = ["kat.npz", "cube64.npz", "fdk_model_bounds.json"]
    if mkl_fftw.available():
        record_mkl()
        files.append("mkl_fft.npz")
    for f in files:
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


def record_mkl():
    """What tests/test_oracle_kat.py's bit-exact checksum test hands MKL: the KAT filter and the 8 weighted projections."""
    det = O.DetectorGeometry(64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 45)
    fs = O.filter_size(det.n_row)
    log = []
    k = mkl_fftw.make_filter(O, fs, det.l_px_row, log=log)
    rf = mkl_fftw.RowFilter(fs, det.n_col, log=log)
    for i in range(8):
        p = O.lcg_projection(det.n_row, det.n_col, i)
        O.weight(p, det)
        rf.apply(p, k)
    mkl_fftw.save_log(log, os.path.join(HERE, "mkl_fft.npz"))


def record_fdk_model_bounds():
    """Per case and stage: the oracle's largest absolute error against the float64 model relative to the model's largest magnitude,
    and the share of voxels that needed the boundary rule. The errors are rounded UP to three significant digits, so that another
    BLAS's float64 summation order in the model cannot move a figure past its record."""
    import fdk_cases

    def up(x):
        q = 10.0 ** (math.floor(math.log10(x)) - 2)
        return float("%.2e" % (math.ceil(x / q) * q))

    bounds = {case: {stage: {"error": up(err), "boundary_share": share} for stage, (err, share) in fdk_cases.oracle_errors(O, case).items()}
              for case in fdk_cases.ORACLE_CASES}
    with open(os.path.join(HERE, fdk_cases.BOUNDS_FILE), "w") as f:
        json.dump(bounds, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1:] == ["fdk_model_bounds"]:
        record_fdk_model_bounds()
    else:
        main()
