"""The device memory a ctx keeps for its settings, all settings together on one ctx: what
paris_hip_projection_reserve_bytes counts for each alone and for all at once, that every clear gives it back, and that a destroy
with every setting in force and their passes still queued releases it all.

Ten of the twelve settings can be cleared (for the two sequences and the lag state "clear" is discard or end). The volume export's
counters and its staging buffer cannot: the library has no call that gives them up before the ctx goes. They are therefore measured
last, stay in place from then on, and their release is what the destroy at the end shows."""
import numpy as np
import pytest

from paris_amd import _lib
from paris_amd import backend as B
from test_gpu_flat_field import assert_formula, counts, expected, read, references

pytestmark = pytest.mark.gpu

DIM_X, DIM_Y = 96, 80                   # not a multiple of 64 in either direction
DET = B.DetectorGeometry(DIM_X, DIM_Y, 0.2, 0.25, 1.5, -0.75, 100, 200, 90.0)
LAG_MODEL = [(0.05, 0.3), (0.01, 0.02)]
AXIS_FRAMES = 4


class Settings:
    """the twelve settings on one backend: name -> (set, clear); the frames their passes run on"""

    def __init__(self, be):
        self.be = be
        rng = np.random.default_rng(12)
        self.dark, self.flat = references(DIM_Y, DIM_X, 3, 65535.0)
        self.frame = counts(np.float32, self.dark, self.flat, 4, 1e-5)
        self.d = B.load(be, B.Projection(self.frame.copy(), DIM_X, DIM_Y))
        self.d_filter = B.load(be, B.Projection(self.frame.copy(), DIM_X, DIM_Y))
        self.src = B.load(be, B.Projection(rng.uniform(100, 60000, (2 * DIM_Y, 2 * DIM_X)).astype(np.float32), 2 * DIM_X, 2 * DIM_Y))
        self.binned = be.make_projection_device(DIM_X, DIM_Y)
        self.v = be.make_volume_device(8, 8, 8)
        self.q = be.make_volume_device(8, 8, 8)          # 2048 bytes: room for 512 quantised voxels
        self.defects = np.zeros((DIM_Y, DIM_X), np.uint8)
        self.defects[40, 50] = 1                         # one pixel with good neighbours: repairable
        self.bin_mask = (rng.random((2 * DIM_Y, 2 * DIM_X)) < 0.01).astype(np.uint8)
        self.air_mask = np.zeros((DIM_Y, DIM_X), np.uint8)
        self.air_mask[2, 3] = 1
        self.c = np.where(rng.random((DIM_Y, DIM_X)) < 0.05, np.float32(0.5), np.float32(0))
        be.set_lag_correction(LAG_MODEL)                 # the model owns nothing on the device: the open sequence does
        self.clearable = {
            "flat field": (lambda: be.set_flat_field(self.dark, self.flat), be.clear_flat_field),
            "defect map": (lambda: be.set_defect_map(self.defects), be.clear_defect_map),
            "zinger filter": (lambda: be.set_zinger_filter(50.0, 0.0, "both", DIM_X, DIM_Y), be.clear_zinger_filter),
            "ring profile": (lambda: be.ring_profile_begin(DIM_X, DIM_Y), be.ring_profile_discard),
            "ring correction": (lambda: be.set_ring_correction(self.c), be.clear_ring_correction),
            "axis search": (lambda: be.axis_search_begin(-1.0, 1.0, 3, DET, AXIS_FRAMES, rows=2), be.axis_search_discard),
            "binning": (lambda: be.set_binning(2, 2, 2 * DIM_X, 2 * DIM_Y, self.bin_mask), be.clear_binning),
            "air region": (lambda: be.set_air_region(0, 0, 8, 8, DIM_X, DIM_Y, mask=self.air_mask), be.clear_air_region),
            "lag sequence": (lambda: be.lag_begin(DIM_X, DIM_Y), be.lag_end),
            "row extension": (self.set_row_extension, be.clear_row_extension),
        }
        self.permanent = {
            "export counters": lambda: be.quantize_volume(self.v, 0.0, 1.0, np.uint8, out=self.q),
            "export staging": lambda: be.quantize_volume(self.v, 0.0, 1.0, np.uint8),
        }

    def set_row_extension(self):
        """the setting, and one filter call that caches a response"""
        self.be.set_row_extension(4, 16)
        B.weight(self.be, self.d_filter, DET)
        B.filter(self.be, self.d_filter, DET)

    def reserve(self):
        return self.be.projection_reserve_bytes(DIM_X, DIM_Y)

    def set_all(self):
        for name in self.clearable:
            self.clearable[name][0]()
        for name in self.permanent:
            self.permanent[name]()

    def queue_passes(self):
        """one pass of each kind on the frames, nothing waited for"""
        be, d = self.be, self.d
        be.bin_frames(self.src, self.binned)
        be.lag_correct(d)
        be.flat_field_rows(d)
        be.air_normalize(d)
        be.defect_repair_rows(d)
        be.zinger_filter_rows(d)
        be.ring_profile_add_rows(d)
        be.ring_correct_rows(d)
        be.axis_search_add(d, 0)
        B.weight(be, self.d_filter, DET)
        B.filter(be, self.d_filter, DET)
        be.quantize_volume(self.v, 0.0, 1.0, np.uint8, out=self.q)


def test_the_settings_held_together_are_counted_cleared_and_released_by_destroy():
    with B.Backend(0, synchronous=False) as abe:
        s = Settings(abe)
        base = s.reserve()
        # each setting alone
        delta = {}
        for name, (put, clear) in s.clearable.items():
            put()
            delta[name] = s.reserve() - base
            if name == "defect map":
                assert delta[name] == abe.defect_map_info().device_bytes
            clear()
            assert s.reserve() == base, name
        for name, put in s.permanent.items():
            before = s.reserve()
            put()
            delta[name] = s.reserve() - before
        print("reserve deltas:", delta)
        assert len(delta) == 12 and all(v > 0 for v in delta.values()), delta
        px = DIM_X * DIM_Y
        assert delta["flat field"] == 8 * px and delta["ring profile"] == 8 * px and delta["ring correction"] == 4 * px
        assert delta["binning"] == 4 * px and delta["lag sequence"] == len(LAG_MODEL) * 4 * px and delta["row extension"] == 4 * DIM_X
        assert delta["export counters"] == 64 + 8 * _lib.VOLUME_HISTOGRAM_BINS_MAX and delta["export staging"] == 512
        kept = delta["export counters"] + delta["export staging"]
        assert s.reserve() == base + kept
        # all twelve on one ctx, cleared in another order
        s.set_all()
        assert s.reserve() == base + sum(delta.values())
        order = ["air region", "flat field", "row extension", "ring correction", "lag sequence", "axis search", "zinger filter", "binning",
                 "ring profile", "defect map"]
        assert sorted(order) == sorted(s.clearable) and order != list(s.clearable)
        left = sum(delta.values())
        for name in order:
            s.clearable[name][1]()
            left -= delta[name]
            assert s.reserve() == base + left, name
        assert s.reserve() == base + kept
        # all twelve again, a pass of each kind queued, nothing cleared or waited for: the destroy releases it all
        s.set_all()
        assert s.reserve() == base + sum(delta.values())
        s.queue_passes()
    with B.Backend(0, synchronous=False) as abe:
        assert abe.projection_reserve_bytes(DIM_X, DIM_Y) == base
        dark, flat = references(DIM_Y, DIM_X, 5, 65535.0)
        frame = counts(np.float32, dark, flat, 6, 1e-5)
        abe.set_flat_field(dark, flat)
        d = B.load(abe, B.Projection(frame.copy(), DIM_X, DIM_Y))
        abe.flat_field_rows(d)
        assert_formula(read(abe, d), expected(frame, dark, flat, 1e-5), "a fresh ctx after the destroy")
