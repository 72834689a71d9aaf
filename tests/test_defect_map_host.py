"""The repair plan of a detector defect map (paris_hip_defect_plan_*) against a numpy float64 restatement of
the rule. Host only: the plan builder needs no device, and it is the only implementation of the rule -- the device just walks it."""
import ctypes as C

import numpy as np
import pytest

import defect_rule as R
from paris_amd import _lib
from paris_amd import backend as B


@pytest.fixture(scope="module")
def case():
    mask = R.shared_mask()
    return mask, B.defect_plan(mask), R.restate(mask)


def test_the_mask_holds_every_case_the_rule_distinguishes(case):
    mask, plan, (defect, first, source, weight, lost, reach_r, reach_c) = case
    assert mask.shape == (80, 96)
    n_src = dict(zip(defect.tolist(), np.diff(first).tolist()))
    ring = {q: int(np.abs(source[first[k]:first[k + 1]] // 96 - q // 96).max()) for k, q in enumerate(defect.tolist())}
    assert n_src[5 * 96 + 7] == 8                       # isolated: the whole ring 1
    assert n_src[0] == 3 and n_src[79 * 96 + 95] == 3   # corners: ring 1 clipped to the detector
    assert n_src[10 * 96 + 20] == 5                     # 2 x 2 cluster: ring 1 less the three other members
    assert ring[22 * 96 + 52] == 3                      # the centre of the 5 x 5 block
    assert 59 * 96 + 69 in lost.tolist() and len(lost) == 9   # the middle 3 x 3 of the 19 x 19 block
    assert n_src[30 * 96 + 40] == 4                     # where the dead row and column cross: the four diagonal neighbours
    assert reach_r == 8 and reach_c == 8


def test_lists_counts_and_reach_are_the_restatement_s(case):
    mask, plan, (defect, first, source, weight, lost, reach_r, reach_c) = case
    assert plan.defect.dtype == np.uint32 and plan.weight.dtype == np.float32
    assert np.array_equal(plan.defect, defect)
    assert np.all(np.diff(plan.defect.astype(np.int64)) > 0)   # sorted row-major
    assert np.array_equal(plan.first_source, first)
    assert np.array_equal(plan.source, source)
    assert plan.defects == np.count_nonzero(mask) and plan.unrepairable == len(lost) and plan.sources == len(source)
    marked = np.flatnonzero(mask.reshape(-1))
    assert np.array_equal(np.setdiff1d(marked, plan.defect), lost)   # the unrepairable set
    assert (plan.reach_rows, plan.reach_cols) == (reach_r, reach_c)
    assert not mask.reshape(-1)[plan.source].any()   # sources are good pixels only
    assert plan.device_bytes == 4 * (2 * len(defect) + 1 + 2 * len(source))


def test_weights_within_one_ulp_and_summing_to_one(case):
    mask, plan, (defect, first, source, weight, lost, reach_r, reach_c) = case
    w32 = weight.astype(np.float32)
    ulp = np.spacing(np.abs(w32)).astype(np.float64)
    assert np.all(np.abs(plan.weight.astype(np.float64) - weight) <= ulp)
    assert np.all(plan.weight > 0)
    for k in range(len(defect)):
        w = plan.weight[first[k]:first[k + 1]].astype(np.float64)
        assert abs(w.sum() - 1.0) <= len(w) * 2.0 ** -24, (k, w.sum())


def test_all_good_and_all_defective_masks():
    empty = B.defect_plan(np.zeros((80, 96), np.uint8))
    assert (empty.defects, empty.unrepairable, empty.sources, empty.reach_rows, empty.reach_cols, empty.device_bytes) == (0,) * 6
    assert len(empty.defect) == 0 and len(empty.source) == 0 and empty.first_source.tolist() == [0]
    full = B.defect_plan(np.ones((80, 96), np.uint8))
    assert full.defects == full.unrepairable == 80 * 96 and full.sources == 0 and len(full.defect) == 0
    assert full.first_source.tolist() == [0] and full.device_bytes == 0


def test_small_and_degenerate_detectors():
    one = B.defect_plan(np.ones((1, 1), np.uint8))
    assert one.defects == 1 and one.unrepairable == 1
    row = np.zeros((1, 20), np.uint8)
    row[0, 3:12] = 1   # a 1-row detector: sources to the left and right only, the middle pixel's at distance 5
    plan, want = B.defect_plan(row), R.restate(row)
    assert np.array_equal(plan.defect, want[0]) and np.array_equal(plan.source, want[2])
    assert plan.reach_rows == 0 and plan.reach_cols == 5


def test_refusals():
    L = _lib.load()
    m = np.zeros((4, 4), np.uint8)
    plan = C.c_void_p()
    assert L.paris_hip_defect_plan_create(None, 4, 4, C.byref(plan)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_defect_plan_create(m.ctypes.data, 0, 4, C.byref(plan)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_defect_plan_create(m.ctypes.data, 4, 0, C.byref(plan)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_defect_plan_create(m.ctypes.data, 4, 4, None) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_defect_plan_stats(None, C.byref(_lib.DefectStats())) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_defect_plan_destroy(None) == 0
    with pytest.raises(ValueError):
        B.defect_plan(np.zeros(16, np.uint8))


def test_quality_figures_of_the_oracle(oracle):
    """calibrates tests/test_gpu_defect_map.py: the float64 restatement of the repair (with the plan's fp32 weights, rounded once to
    fp32) and the oracle's weight, filter and backprojection at the 64 x 48 driver geometry, against the clean reconstruction"""
    det = oracle.DetectorGeometry(*R.QUALITY_GEO)
    vg = oracle.calculate_volume_geometry(det)
    lines = R.quality_frames(vg.dim_x, vg.l_vx_x)
    mask = R.quality_mask()
    plan = B.defect_plan(mask)
    assert plan.defects == 130 and plan.unrepairable == 0
    clean = oracle.reconstruct(det, vg, len(lines), projections=lines)
    zeroed = [np.where(mask != 0, np.float32(0), p) for p in lines]
    repaired = [R.repair64(z, plan.defect, plan.first_source, plan.source, plan.weight)[0].astype(np.float32) for z in zeroed]
    a = R.relative_rms(oracle.reconstruct(det, vg, len(lines), projections=zeroed), clean)
    b = R.relative_rms(oracle.reconstruct(det, vg, len(lines), projections=repaired), clean)
    print("defect map quality (oracle): relative RMS %.4g with the dead pixels at 0, %.4g repaired" % (a, b))
    assert a == pytest.approx(R.CAL_ZEROED, rel=0.02) and b == pytest.approx(R.CAL_REPAIRED, rel=0.02)
    assert b < a / 5
