"""The driver's row plan (paris_amd/host/paris/frame_rows.h: plan_frame_rows) against its restatement,
chain_rule.band_rows, which tests/test_gpu_frame_chain.py runs the passes with: the C++ the driver is built from, through
demo/paris_hip_frame_rows, for every band of two detectors under every setting that moves a range. Host only: no ctx, no device."""
import itertools
import os
import subprocess

import pytest

import binning_rule
import chain_rule as CR
from paris_amd import backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "paris_amd", "host", "demo", "paris_hip_frame_rows")

# dim_y -> the detector with that many rows: the chain tests' detector, and the same binned 2 x 2
GEOS = {45: CR.GEO, 22: binning_rule.binned_geometry(CR.GEO, 2, 2)}
# dim_y -> the air rectangle's (y0, height): none, the chain tests' rows, the detector's last rows
RECTS = {45: (None, (CR.AIR_RECT[1][1], CR.AIR_RECT[1][3]), (42, 3)), 22: (None, (CR.AIR_RECT[2][1], CR.AIR_RECT[2][3]), (19, 3))}
REACH = (0, 4, 8)
ROLLS = (0.0, 0.3, -1.0)      # 0: no roll (the rule refuses it as a setting)


def cases():
    for dim_y in (22, 45):
        bands = [(first, count) for first in range(dim_y + 1) for count in range(dim_y - first + 1)]
        yield from itertools.product((dim_y,), bands, REACH, (False, True), RECTS[dim_y], (1, 2), ROLLS)


@pytest.fixture(scope="module")
def plans():
    """every case with the program's answer: one start of the program for all of them"""
    if not os.path.exists(EXE):
        pytest.fail("%s missing: run __graft_entry__.build()" % EXE)
    all_cases = list(cases())
    lines = []
    for dim_y, band, reach, zingers, rect, bin_y, eta in all_cases:
        geo = " ".join("%d" % v if isinstance(v, int) else "%.9g" % float(v) for v in GEOS[dim_y])
        y0, height = rect if rect is not None else (0, 0)
        lines.append("%s %d %d %d %d %d %d %d %.9g" % (geo, band[0], band[1], reach, zingers, y0, height, bin_y, eta))
    r = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(all_cases)
    return all_cases, got


def test_the_cases_cover_what_moves_a_range():
    all_cases = list(cases())
    assert len(all_cases) == (23 * 24 // 2 + 46 * 47 // 2) * 3 * 2 * 3 * 2 * 3
    assert GEOS[22][:2] == (33, 22) and GEOS[45][:2] == (67, 45)
    assert {c[1] for c in all_cases if c[0] == 22} >= {(0, 0), (22, 0), (0, 22), (21, 1)}
    for dim_y, rects in RECTS.items():
        assert rects[0] is None and all(y0 + h <= dim_y for y0, h in rects[1:]) and rects[2][0] + rects[2][1] == dim_y


def test_every_plan_equals_the_restatement(plans):
    all_cases, got = plans
    source_rows = {}
    checked = rolled = 0
    for (dim_y, band, reach, zingers, rect, bin_y, eta), g in zip(all_cases, got):
        read = band
        if eta != 0.0 and band[1] != 0:
            key = (dim_y, eta, band)
            if key not in source_rows:
                source_rows[key] = B.detector_roll_source_rows(eta, B.DetectorGeometry(*GEOS[dim_y]), *band)
            read = source_rows[key]
            rolled += 1
        want = CR.band_rows(read[0], read[1], dim_y, reach, zingers, None if rect is None else (0, rect[0], 1, rect[1]), bin_y)
        flat = tuple(band) + tuple(want.band) + tuple(want.fix) + tuple(want.air) + tuple(want.up) + tuple(want.src)
        assert g == flat, ((dim_y, band, reach, zingers, rect, bin_y, eta), g, flat)
        checked += 1
    assert checked == len(all_cases) and rolled > checked // 2
    # the roll moves bands: its source range is not the band itself
    assert any(rows != key[2] for key, rows in source_rows.items())
