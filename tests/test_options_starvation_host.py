"""The driver's --starvation P0[:GAIN[:RADIUS]] (paris_amd/host/paris/options.h: parse_starvation in the table of
detail::find_option_parser) through demo/paris_hip_options: the values it accepts with the fields they set, and every value it
refuses. The ranges belong to check_starvation, which needs a detector: tests/test_gpu_starvation_driver.py. Host only: no ctx."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "paris_amd", "host", "demo", "paris_hip_options")
FLAG, USAGE = "--starvation", "--starvation P0[:GAIN[:RADIUS]]"
INF, NAN = math.inf, math.nan

ACCEPTED = [
    ("3.5", dict(starvation=1, starvation_p0=3.5, starvation_gain=1.0, starvation_radius=3)),
    ("3.5:0.5", dict(starvation=1, starvation_p0=3.5, starvation_gain=0.5, starvation_radius=3)),
    ("3.5:2:4", dict(starvation=1, starvation_p0=3.5, starvation_gain=2.0, starvation_radius=4)),
    ("-1e-3:1e50:0", dict(starvation_p0=-1e-3, starvation_gain=INF, starvation_radius=0)),       # read; the check refuses them
    ("nan:-2:007", dict(starvation_p0=NAN, starvation_gain=-2.0, starvation_radius=7)),
    (" 0x1p+1:1e-42:1", dict(starvation_p0=2.0, starvation_gain=1e-42, starvation_radius=1)),
]
REFUSED = ["", ":", "3.5:", ":1", "3.5:1:", "3.5:1:3:", "3.5:1:3:4", "3.5::3", "x", "3.5x", "3.5:y", "3.5:1:z", "3.5:1:3.0", "3.5:1:-3", "3.5:1:+3",
           "3.5 ", "3.5:1:1234567890"]
# another option leaves the fields at their defaults
OTHER = ("--axis-rows", "4", dict(starvation=0, starvation_p0=0.0, starvation_gain=1.0, starvation_radius=3))


@pytest.fixture(scope="module")
def answers():
    if not os.path.exists(EXE):
        pytest.fail("%s missing: run __graft_entry__.build()" % EXE)
    lines = [(FLAG, v) for v, _ in ACCEPTED] + [(FLAG, v) for v in REFUSED] + [OTHER[:2]]
    r = subprocess.run([EXE], input="".join("%s %s\n" % lv for lv in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return dict(zip(lines, out))


def assert_fields(line, want):
    assert not line.startswith("refused"), line
    got = dict(item.split("=", 1) for item in line.split())
    for name, value in want.items():
        if isinstance(value, int):
            assert int(got[name]) == value, (name, got[name], value)
        else:
            g, w = float.fromhex(got[name]), float(np.float32(value))
            assert (math.isnan(g) and math.isnan(w)) or g == w, (name, got[name], w)


@pytest.mark.parametrize("value,want", ACCEPTED)
def test_accepted_values_set_their_fields(answers, value, want):
    assert_fields(answers[(FLAG, value)], want)


@pytest.mark.parametrize("value", REFUSED)
def test_refused_values_name_the_usage(answers, value):
    assert answers[(FLAG, value)] == "refused: %s: cannot read '%s'" % (USAGE, value)


def test_the_defaults_stay_under_another_option(answers):
    assert_fields(answers[OTHER[:2]], OTHER[2])
