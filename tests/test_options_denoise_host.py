"""The driver's parser of --denoise (paris/options.h), value by value through demo/paris_hip_options as
tests/test_options_host.py does for the other options: the fields each spelling sets, the defaults, and the spellings it refuses, each
with its message. Ranges are check_denoise's, which the driver runs (tests/test_gpu_denoise_driver.py). No device."""
import subprocess

import numpy as np
import pytest

from test_options_host import EXE, fields_of

USAGE = "--denoise SIGMA_R[:SIGMA_S[:RADIUS]]"
ACCEPTED = [
    ("--denoise", "0.05", dict(denoise=1, denoise_sigma_r=0.05, denoise_sigma_s=1.0, denoise_radius=2, denoise_radius_given=0)),
    ("--denoise", "0.05:0.4", dict(denoise=1, denoise_sigma_s=0.4, denoise_radius=1)),          # min(3, ceil(0.8))
    ("--denoise", "0.05:0.5", dict(denoise_sigma_s=0.5, denoise_radius=1)),                      # ceil(1.0)
    ("--denoise", "0.05:0.51", dict(denoise_sigma_s=0.51, denoise_radius=2)),
    ("--denoise", "0.05:1.25", dict(denoise_sigma_s=1.25, denoise_radius=3)),                    # ceil(2.5)
    ("--denoise", "0.05:7", dict(denoise_sigma_s=7.0, denoise_radius=3, denoise_radius_given=0)),  # capped
    ("--denoise", "2e3:1.25:1", dict(denoise_sigma_r=2e3, denoise_sigma_s=1.25, denoise_radius=1, denoise_radius_given=1)),
    ("--denoise", "0.05:1:3", dict(denoise_radius=3, denoise_radius_given=1)),
    ("--denoise", "0.05:1:0", dict(denoise=1, denoise_radius=0, denoise_radius_given=1)),        # ranges: check_denoise
    ("--denoise", "0.05:1:17", dict(denoise_radius=17)),
    ("--denoise", "nan:inf", dict(denoise=1, denoise_sigma_r=np.nan, denoise_sigma_s=np.inf, denoise_radius=0)),
    ("--denoise", "-1:-2", dict(denoise_sigma_r=-1.0, denoise_sigma_s=-2.0, denoise_radius=0)),
    ("--denoise", "0x1p-4: 2", dict(denoise_sigma_r=0.0625, denoise_sigma_s=2.0, denoise_radius=3)),   # what strtof reads
]
REFUSED = [
    ("--denoise", ""),
    ("--denoise", ":1"),
    ("--denoise", "0.05:"),
    ("--denoise", "0.05:1:"),
    ("--denoise", "0.05:1:2:3"),
    ("--denoise", "soft"),
    ("--denoise", "0.05mm"),
    ("--denoise", "0.05:1vx"),
    ("--denoise", "0.05:1:2.0"),
    ("--denoise", "0.05:1:-1"),
    ("--denoise", "0.05:1:1e0"),
    ("--denoise", "0.05:1: 2"),
    ("--denoise", "0.05:1:1234567890"),
    ("--denoise", "0.05,1,2"),
]


@pytest.fixture(scope="module")
def answers():
    lines = [(c[0], c[1]) for c in ACCEPTED + REFUSED]
    r = subprocess.run([EXE], input="".join("%s %s\n" % lv for lv in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return dict(zip(lines, out))


@pytest.mark.parametrize("flag,value,want", ACCEPTED, ids=lambda v: v if isinstance(v, str) else "")
def test_accepted_values_set_their_fields(answers, flag, value, want):
    got = fields_of(answers[(flag, value)])
    for name, w in want.items():
        if isinstance(w, int):
            assert int(got[name]) == w, (name, got[name])
        else:
            g = float.fromhex(got[name])
            assert (np.isnan(g) and np.isnan(w)) or g == float(np.float32(w)), (name, got[name])


@pytest.mark.parametrize("flag,value", REFUSED, ids=lambda v: v)
def test_refused_values_name_the_usage(answers, flag, value):
    assert answers[(flag, value)] == "refused: %s: cannot read '%s'" % (USAGE, value)


def test_other_options_leave_it_off(answers):
    r = subprocess.run([EXE], input="--metal 1.5\n", capture_output=True, text=True, timeout=60)
    got = fields_of(r.stdout.splitlines()[0])
    assert int(got["denoise"]) == 0 and float.fromhex(got["denoise_sigma_s"]) == 1.0 and int(got["denoise_radius"]) == 0
