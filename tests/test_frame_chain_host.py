"""The scan and the composed rule of tests/chain_rule.py, on the CPU: every pass of the chain changes bits of the final frames, no frame
saturates the zinger filter, the ring correction is not all zero and every frame is air-normalised -- so the equalities of the GPU chain
tests (tests/test_gpu_frame_chain.py, tests/test_gpu_chain_driver.py) cannot be met by passes that do nothing --, the stacked repair
equals binning_rule.repair32, and the band rule gives the ranges worked out by hand."""
import numpy as np
import pytest

import binning_rule
import chain_rule as CH
import ring_rule


@pytest.fixture(scope="module")
def scan():
    return CH.scan()


@pytest.fixture(scope="module", params=[1, 2], ids=["unbinned", "bin2"])
def run(request, scan):
    st = CH.settings(scan, request.param)
    steps, info = CH.chain(scan.counts, st)
    return st, steps, info


def test_every_pass_changes_bits_of_the_final_frames(scan, run):
    CH.assert_every_pass_counts(scan.counts, *run)


def test_the_passes_do_what_the_scan_was_made_for(scan, run):
    st, steps, info = run
    # the air values are the frames' drift, -ln(1 + e_f), but for the few offsets and zingers that fall into the rectangle
    assert np.corrcoef(info.air, -np.log1p(scan.eps))[0, 1] > 0.95 and np.ptp(info.air) > 0.09
    # the correction finds the planted column (a third of the way along the rows) where the phantom's own structure leaves it above
    # the floor, and with it the offsets' size
    if st.bin == 1:
        found = info.ring_c[:, CH.GEO[0] // 3]
        assert np.count_nonzero(found) > 15 and abs(np.median(found[found != 0]) - ring_rule.OFFSET) < 0.01
    # a swapped order is another rule: the composed frames tell
    order = list(CH.STEPS)
    order[3], order[4] = order[4], order[3]
    assert not np.array_equal(CH.bits(CH.chain(scan.counts, st, order=order)[0][-1]), CH.bits(steps[-1]))


def test_the_stacked_repair_equals_the_single_frame_rule(scan, run):
    st, steps, _ = run
    before = steps[3][:2]
    got = CH.repair(before, st.plan)
    for k in range(2):
        assert np.array_equal(CH.bits(got[k]), CH.bits(binning_rule.repair32(before[k], st.plan)))


def test_the_band_rule():
    rect = (54, 1, 12, 6)
    r = CH.band_rows(20, 5, 45, 4, True, rect, 1)
    assert (r.band, r.fix, r.air, r.up, r.src) == ((20, 5), (19, 7), (15, 15), (1, 29), (1, 29))
    r = CH.band_rows(20, 5, 45, 4, True, None, 2)
    assert (r.fix, r.air, r.up, r.src) == ((19, 7), (15, 15), (15, 15), (30, 30))
    r = CH.band_rows(0, 1, 45, 4, True, rect, 1)
    assert (r.fix, r.air, r.up) == ((0, 2), (0, 6), (0, 7))
    r = CH.band_rows(44, 1, 45, 4, False, rect, 1)
    assert (r.fix, r.air, r.up) == ((44, 1), (40, 5), (1, 44))
    r = CH.band_rows(0, 45, 45, 4, True, rect, 1)
    assert (r.fix, r.air, r.up) == ((0, 45), (0, 45), (0, 45))
    r = CH.band_rows(7, 0, 45, 4, True, rect, 2)
    assert (r.band, r.fix, r.air, r.up, r.src) == ((7, 0), (7, 0), (7, 0), (7, 0), (14, 0))
