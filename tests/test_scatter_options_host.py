"""The driver's parsers of --scatter, --scatter-iterations, --scatter-limit and --scatter-margin (paris/options.h, DESIGN.md section
4.23), value by value through demo/paris_hip_options as tests/test_options_host.py does for the other options: the fields they set, the
defaults they leave, and the spellings they refuse. Ranges are check_scatter's, which needs the detector
(tests/test_gpu_scatter_driver.py). No device."""
import subprocess

import numpy as np
import pytest

from test_options_host import EXE, fields_of

USAGE = "--scatter A:ALPHA:BETA:SIGMA1_MM[:SIGMA2_MM:W2]"
ACCEPTED = [
    ("--scatter", "0.05:-0.15:1:0.6:2:0.5", dict(scatter=1, scatter_amplitude=0.05, scatter_alpha=-0.15, scatter_beta=1.0, scatter_sigma1=0.6,
                                                 scatter_sigma2=2.0, scatter_weight2=0.5, scatter_limit=0.8, scatter_iterations=4, scatter_margin=0,
                                                 scatter_detail_given=0)),
    ("--scatter", "0.3:0.25:0.5:0.6", dict(scatter=1, scatter_amplitude=0.3, scatter_sigma1=0.6, scatter_sigma2=0.6, scatter_weight2=0.0)),
    ("--scatter", "nan:3:-1:0:inf:-2", dict(scatter=1, scatter_amplitude=np.nan, scatter_alpha=3.0, scatter_sigma2=np.inf)),   # ranges: check_scatter
    ("--scatter-iterations", "16", dict(scatter=0, scatter_iterations=16, scatter_detail_given=1)),
    ("--scatter-iterations", "0", dict(scatter_iterations=0, scatter_detail_given=1)),
    ("--scatter-limit", "0.25", dict(scatter=0, scatter_limit=0.25, scatter_detail_given=1)),
    ("--scatter-margin", "1024", dict(scatter=0, scatter_margin=1024, scatter_detail_given=1)),
]
REFUSED = [
    ("--scatter", "", "%s: cannot read ''" % USAGE),
    ("--scatter", "0.05:-0.15:1", "%s: cannot read '0.05:-0.15:1'" % USAGE),
    ("--scatter", "0.05:-0.15:1:0.6:2", "%s: cannot read '0.05:-0.15:1:0.6:2'" % USAGE),
    ("--scatter", "0.05:-0.15:1:0.6:2:0.5:7", "%s: cannot read '0.05:-0.15:1:0.6:2:0.5:7'" % USAGE),
    ("--scatter", "0.05:-0.15:1:wide", "%s: cannot read '0.05:-0.15:1:wide'" % USAGE),
    ("--scatter", "0.05:-0.15:1:0.6mm", "%s: cannot read '0.05:-0.15:1:0.6mm'" % USAGE),
    ("--scatter-iterations", "2.5", "--scatter-iterations N: cannot read '2.5'"),
    ("--scatter-iterations", "-1", "--scatter-iterations N: cannot read '-1'"),
    ("--scatter-limit", "half", "--scatter-limit F: cannot read 'half'"),
    ("--scatter-margin", "0", "--scatter-margin M: M must lie in 1 .. 1024"),
    ("--scatter-margin", "12px", "--scatter-margin M: cannot read '12px'"),
]


@pytest.fixture(scope="module")
def answers():
    lines = [(f, v) for f, v, _ in ACCEPTED + REFUSED]
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


@pytest.mark.parametrize("flag,value,want", REFUSED, ids=lambda v: v if isinstance(v, str) else "")
def test_refused_values_name_the_usage(answers, flag, value, want):
    assert answers[(flag, value)] == "refused: " + want
