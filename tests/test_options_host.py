"""The driver's option parsers (paris_amd/host/paris/options.h: the table of detail::find_option_parser) through demo/paris_hip_options:
for every option of the table, values it accepts with the fields they must set, and values it refuses. The expectations are written
here by hand, from the parsers as they were before they shared their field readers. Host only: no ctx, no device.

Two cases changed with the shared number reader and stand under their own names (OUT_OF_RANGE): text outside a float's range given
to --zingers or --rings was refused as "cannot read" by std::stof; it is now read as every other option always read it -- inf, which
check_zingers / check_rings refuse as not finite, or a subnormal, which is a legal threshold."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "paris_amd", "host", "demo", "paris_hip_options")

# the fields the tool prints as double that are float in program_options: an expectation is rounded to float before it is compared
F32 = {"zinger_abs", "zinger_rel", "ring_floor", "ring_limit", "axis_lo", "axis_hi", "axis_step", "roll_deg", "roll_lo", "roll_hi", "roll_step",
       "air_limit", "phase_alpha", "phase_floor", "bh_c1", "bh_c2", "bh_c3", "bh_c4", "lag_b1", "lag_a1", "lag_b2", "lag_a2", "lag_b3", "lag_a3",
       "lag_b4", "lag_a4", "metal_threshold", "metal_min_path", "voxel_lo", "voxel_hi"}
F64 = {"phase_delta_beta", "phase_energy", "voxel_p_lo", "voxel_p_hi"}
INF, NAN = math.inf, math.nan

# flag -> (usage, the words of its refusal, accepted: [(value, fields)], refused: [value or (value, words)])
OPTIONS = {
    "--bin": ("--bin BX[:BY]", "each factor is 1, 2, 4 or 8", [
        ("2", dict(bin_x=2, bin_y=2)),
        ("4:1", dict(bin_x=4, bin_y=1)),
        ("1:8", dict(bin_x=1, bin_y=8, zingers=0, air=0)),
    ], ["", ":", "2:", ":2", "2:4:8", "3", "x", "2:x", "+2", "02", " 2", "16"]),
    "--zingers": ("--zingers ABS[:REL]", "cannot read", [
        ("0.5", dict(zingers=1, zinger_abs=0.5, zinger_rel=0.0, zinger_polarity=2)),
        ("0.1:0.25", dict(zingers=1, zinger_abs=0.1, zinger_rel=0.25)),
        (" 1.5:-2e3", dict(zinger_abs=1.5, zinger_rel=-2000.0)),
        ("inf:nan", dict(zinger_abs=INF, zinger_rel=NAN)),
        ("0x1p-3", dict(zinger_abs=0.125)),
    ], ["", ":", "0.5:", ":0.5", "1:2:3", "x", "1x", "1 ", "1:2x", "0.5:0.1:"]),
    "--zinger-polarity": ("--zinger-polarity bright|dark|both", "unknown polarity", [
        ("bright", dict(zinger_polarity=1, zingers=0)),
        ("dark", dict(zinger_polarity=-1)),
        ("both", dict(zinger_polarity=0)),
    ], ["", "Bright", "bright:", "up", "1"]),
    "--extend-rows": ("--extend-rows W[:M]", "cannot read", [
        ("16", dict(extend_rows=1, extend_taper=16, extend_edge=4)),
        ("16:2", dict(extend_rows=1, extend_taper=16, extend_edge=2)),
        ("123456789:007", dict(extend_taper=123456789, extend_edge=7)),
    ], ["", ":", "16:", ":2", "1:2:3", "x", "1x", "+1", "-1", "1.5", "1234567890", "16:1234567890", " 16"]),
    "--rings": ("--rings H[:FLOOR[:LIMIT]]", "cannot read", [
        ("3", dict(rings=1, ring_half_width=3, ring_floor=0.0, ring_limit=0.0)),
        ("3:0.01", dict(rings=1, ring_half_width=3, ring_floor=0.01, ring_limit=0.0)),
        ("32:0.01:2.5", dict(ring_half_width=32, ring_floor=0.01, ring_limit=2.5)),
        ("1:inf:-1", dict(ring_floor=INF, ring_limit=-1.0)),
    ], ["", ":", ":0.1", "3:", "3:0.1:", "3:0.1:2:4", "3::1", "x", "3:x", "3:0.1:y", "+3", "-3", "3.0", "1234567890"]),
    "--find-axis": ("--find-axis LO:HI[:STEP]", "cannot read", [
        ("-2:2", dict(find_axis=1, axis_lo=-2.0, axis_hi=2.0, axis_step=0.25)),
        ("-2.5:2.5:0.5", dict(find_axis=1, axis_lo=-2.5, axis_hi=2.5, axis_step=0.5)),
        ("1e50:1e-42:nan", dict(axis_lo=INF, axis_hi=1e-42, axis_step=NAN, axis_rows=2, axis_rows_given=0)),
    ], ["", "1", "1:", ":1", ":", "1:2:", "1:2:3:4", "a:1", "1:2x", "1::3", "1: "]),
    "--axis-rows": ("--axis-rows R", "cannot read", [
        ("4", dict(axis_rows=4, axis_rows_given=1, find_axis=0)),
        ("064", dict(axis_rows=64)),
    ], ["", "x", "+4", "-4", "4:", "4:2", ":4", "1234567890", "4.0"]),
    "--detector-roll": ("--detector-roll DEG", "cannot read", [
        ("0.5", dict(roll=1, roll_deg=0.5, find_roll=0)),
        ("-1.25e0", dict(roll=1, roll_deg=-1.25)),
        ("1e50", dict(roll_deg=INF)),
    ], ["", "x", "0.5x", "0.5:", "0.5:1", ":0.5", " "]),
    "--find-roll": ("--find-roll LO:HI[:STEP]", "cannot read", [
        ("-1:1", dict(find_roll=1, roll_lo=-1.0, roll_hi=1.0, roll_step=0.25, roll=0)),
        ("-1:1:0.125", dict(find_roll=1, roll_lo=-1.0, roll_hi=1.0, roll_step=0.125)),
    ], ["", "1", "1:", ":1", "1:2:", "1:2:3:4", "a:1", "1:2x", "1::3"]),
    "--air-region": ("--air-region X0:Y0:W:H[:LIMIT]", "cannot read", [
        ("1:2:3:4", dict(air=1, air_x0=1, air_y0=2, air_width=3, air_height=4, air_limit=0.0)),
        ("0:40:64:8:0.5", dict(air=1, air_x0=0, air_y0=40, air_width=64, air_height=8, air_limit=0.5)),
        ("1:2:3:4:inf", dict(air_limit=INF)),
    ], ["", "1", "1:2:3", "1:2:3:", "1:2:3:4:", "1:2:3:4:5:6", "1::3:4", "1:2:3:x", "1:2:3:4:x", "-1:2:3:4", "1:+2:3:4", "1:2:3:1234567890",
        "1:2:3.0:4"]),
    "--phase": ("--phase DELTA_BETA:ENERGY_KEV[:MARGIN]", "cannot read", [
        ("1000:25", dict(phase=1, phase_material=1, phase_delta_beta=1000.0, phase_energy=25.0, phase_margin=0, phase_alpha=0.0)),
        ("1e3:25.5:8", dict(phase=1, phase_material=1, phase_delta_beta=1000.0, phase_energy=25.5, phase_margin=8)),
        ("1e-50:1e300", dict(phase_delta_beta=1e-50, phase_energy=1e300, phase_floor_given=0)),
    ], ["", "1000", "1000:", ":25", "1000:25:", "1000:25:8:1", "x:25", "1000:y", "1000:25:+8", "1000:25:1234567890", "1000:25:8.0",
        ("1000:25:0", "MARGIN must lie in 1 .. 1024"), ("1000:25:000", "MARGIN must lie in 1 .. 1024")]),
    "--phase-alpha": ("--phase-alpha MM2[:MARGIN]", "cannot read", [
        ("0.5", dict(phase=1, phase_material=0, phase_alpha=0.5, phase_delta_beta=0.5, phase_energy=0.0, phase_margin=0)),
        ("0.1:16", dict(phase=1, phase_material=0, phase_alpha=0.1, phase_delta_beta=0.1, phase_margin=16)),
        ("1e-50", dict(phase_alpha=0.0, phase_delta_beta=1e-50)),
    ], ["", ":", "0.5:", ":8", "0.5:8:1", "x", "0.5:x", "0.5:-8", ("0.5:0", "MARGIN must lie in 1 .. 1024")]),
    "--phase-floor": ("--phase-floor T", "cannot read", [
        ("0.001", dict(phase_floor_given=1, phase_floor=0.001, phase=0)),
        ("1e-42", dict(phase_floor=1e-42)),
    ], ["", "x", "0.1:", "0.1:2", "0.1x"]),
    "--beam-hardening": ("--beam-hardening C1:C2[:C3[:C4]]", "cannot read", [
        ("1:0.1", dict(beam_hardening=1, bh_degree=2, bh_c1=1.0, bh_c2=0.1, bh_c3=0.0, bh_c4=0.0, fit_beam_hardening=0)),
        ("1:0.1:-0.01", dict(bh_degree=3, bh_c3=-0.01, bh_c4=0.0)),
        ("1:0.1:0.01:1e-3", dict(bh_degree=4, bh_c1=1.0, bh_c2=0.1, bh_c3=0.01, bh_c4=0.001, bh_slices=32, bh_margin=2)),
    ], ["", "1", "1:", ":1", "1:2:", "1:2:3:4:5", "1:x", "1::3", "1:2:3:4:"]),
    "--fit-beam-hardening": ("--fit-beam-hardening N[:SLICES[:MARGIN]]", "cannot read", [
        ("2", dict(fit_beam_hardening=1, bh_degree=2, bh_slices=32, bh_margin=2, beam_hardening=0)),
        ("3:8", dict(fit_beam_hardening=1, bh_degree=3, bh_slices=8, bh_margin=2)),
        ("4:16:0", dict(bh_degree=4, bh_slices=16, bh_margin=0, bh_c1=0.0)),
    ], ["", ":", "2:", ":8", "2:8:", "2:8:0:1", "x", "2:x", "-2", "+2", "2.0", "1234567890", "2:8:1234567890"]),
    "--lag": ("--lag B1:A1[:B2:A2[:B3:A3[:B4:A4]]]", "cannot read", [
        ("0.02:0.5", dict(lag=1, lag_terms=1, lag_b1=0.02, lag_a1=0.5, lag_b2=0.0, lag_a2=0.0, lag_start=1, lag_start_given=0)),
        ("0.02:0.5:0.01:0.05", dict(lag_terms=2, lag_b2=0.01, lag_a2=0.05, lag_b3=0.0)),
        ("0.02:0.5:0.01:0.05:0.003:0.01:1e-3:2e-3", dict(lag_terms=4, lag_b1=0.02, lag_a1=0.5, lag_b2=0.01, lag_a2=0.05, lag_b3=0.003, lag_a3=0.01,
                                                       lag_b4=0.001, lag_a4=0.002)),
    ], ["", "0.01", "0.01:", ":0.5", "0.01:0.5:", "0.01:0.5:0.02", "1:2:3:4:5:6:7:8:9:10", "1:2:3:4:5:6:7:8:9", "0.01:x", "0.01::0.5:0.1"]),
    "--lag-start": ("--lag-start rest|steady", "unknown start", [
        ("rest", dict(lag_start=0, lag_start_given=1, lag=0)),
        ("steady", dict(lag_start=1, lag_start_given=1)),
    ], ["", "warm", "rest:", "Rest"]),
    "--metal": ("--metal THR[:GROW[:MIN_PATH]]", "cannot read", [
        ("0.3", dict(metal=1, metal_threshold=0.3, metal_grow=1, metal_min_path=-1.0)),
        ("0.3:2", dict(metal=1, metal_threshold=0.3, metal_grow=2, metal_min_path=-1.0)),
        ("0.3:0:0.25", dict(metal_grow=0, metal_min_path=0.25)),
        ("nan:2.0:inf", dict(metal_threshold=NAN, metal_grow=2, metal_min_path=INF)),
        ("-1e30:1e6:0", dict(metal_threshold=-1e30, metal_grow=1000000, metal_min_path=0.0)),
        ("1:-0", dict(metal_grow=0)),
    ], ["", ":", "0.3:", ":1", "0.3:1:", "0.3:1:0.25:7", "much", "0.3:1.5", "0.3:-1", "0.3:1e7", "0.3:inf", "0.3:nan", "0.3:x", "0.3:1:x",
        ("0.3:1:-0.5", "MIN_PATH must be finite and not negative (got -0.5)"), ("0.3:1:nan", "MIN_PATH must be finite and not negative")]),
    "--voxel-type": ("--voxel-type u8|u16", "unknown type", [
        ("u8", dict(voxel_type=1, voxel_range_given=0)),
        ("u16", dict(voxel_type=2)),
    ], ["", "u32", "U8", "u8:", "8"]),
    "--voxel-range": ("--voxel-range LO:HI | auto[:P_LO:P_HI]", "cannot read", [
        ("0:1", dict(voxel_range_given=1, voxel_automatic=0, voxel_lo=0.0, voxel_hi=1.0, voxel_type=0)),
        ("-0.01:0.1", dict(voxel_lo=-0.01, voxel_hi=0.1, voxel_p_lo=0.1, voxel_p_hi=99.9)),
        ("auto", dict(voxel_range_given=1, voxel_automatic=1, voxel_p_lo=0.1, voxel_p_hi=99.9, voxel_lo=0.0, voxel_hi=0.0)),
        ("auto:1:99.5", dict(voxel_range_given=1, voxel_automatic=1, voxel_p_lo=1.0, voxel_p_hi=99.5)),
    ], ["", ":", "0", "0:", ":1", "0:1:", "0:1:2", "auto:", "auto:1", "auto:1:", "auto:1:99:5", "auto::99", "x:1", "0:1x", "Auto", "auto:x:99"]),
}

# text outside a float's range: --zingers and --rings read it as every other option does (the one change of the shared number reader)
OUT_OF_RANGE = {
    "overflow_is_inf": [("--zingers", "1e50", dict(zingers=1, zinger_abs=INF, zinger_rel=0.0)),
                        ("--zingers", "1:-1e50", dict(zinger_abs=1.0, zinger_rel=-INF)),
                        ("--rings", "3:1e50", dict(rings=1, ring_half_width=3, ring_floor=INF, ring_limit=0.0)),
                        ("--rings", "3:0:1e50", dict(ring_floor=0.0, ring_limit=INF))],
    "a_subnormal_is_a_threshold": [("--zingers", "1e-42", dict(zingers=1, zinger_abs=1e-42, zinger_rel=0.0)),
                                   ("--zingers", "0:1e-42", dict(zinger_abs=0.0, zinger_rel=1e-42)),
                                   ("--rings", "3:1e-42", dict(rings=1, ring_floor=1e-42)),
                                   ("--rings", "3:0:1e-50", dict(ring_floor=0.0, ring_limit=0.0))],
}


def all_lines():
    lines = []
    for flag, (_, _, accepted, refused) in OPTIONS.items():
        lines += [(flag, value) for value, _ in accepted]
        lines += [(flag, r if isinstance(r, str) else r[0]) for r in refused]
    for cases in OUT_OF_RANGE.values():
        lines += [(flag, value) for flag, value, _ in cases]
    lines.append(("--no-such-option", "1"))
    return lines


@pytest.fixture(scope="module")
def answers():
    """(flag, value) -> the tool's line: one start of the program for every case of this file"""
    if not os.path.exists(EXE):
        pytest.fail("%s missing: run __graft_entry__.build()" % EXE)
    lines = all_lines()
    r = subprocess.run([EXE], input="".join("%s %s\n" % lv for lv in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return dict(zip(lines, out))


def fields_of(line):
    assert not line.startswith("refused"), line
    return dict(item.split("=", 1) for item in line.split())


def assert_fields(line, want, case):
    got = fields_of(line)
    for name, value in want.items():
        if name in F32 or name in F64:
            g = float.fromhex(got[name])
            w = float(np.float32(value)) if name in F32 else float(value)
            assert (math.isnan(g) and math.isnan(w)) or (g == w and math.copysign(1.0, g) == math.copysign(1.0, w)), (case, name, got[name], w)
        else:
            assert isinstance(value, int) and int(got[name]) == value, (case, name, got[name], value)


def test_the_tables_cover_what_the_issue_names():
    assert len(OPTIONS) == 20
    for flag, (usage, _, accepted, refused) in OPTIONS.items():
        assert usage.startswith(flag + " ") and len(accepted) >= 2
        values = [r if isinstance(r, str) else r[0] for r in refused]
        assert "" in values and len(set(values)) == len(values)
        if ":" in usage or "[" in usage:                       # an option of fields: a trailing colon, one field too many
            assert any(v.endswith(":") for v in values)
    assert set(F32).isdisjoint(F64)


def test_defaults_stay_where_no_option_sets_them(answers):
    """a parser touches its own fields only: under an option that belongs to another group, every field holds its default"""
    got = fields_of(answers[("--axis-rows", "4")])
    defaults = dict(bin_x=1, bin_y=1, zingers=0, zinger_polarity=2, extend_rows=0, extend_edge=4, rings=0, find_axis=0, roll=0, find_roll=0, air=0,
                    phase=0, phase_margin=0, phase_floor_given=0, beam_hardening=0, fit_beam_hardening=0, bh_degree=0, bh_slices=32, bh_margin=2, lag=0,
                    lag_terms=0, lag_start=1, lag_start_given=0, metal=0, metal_grow=1, voxel_type=0, voxel_range_given=0, voxel_automatic=0)
    for name, value in defaults.items():
        assert int(got[name]) == value, name
    for name, value in dict(axis_step=0.25, roll_step=0.25, metal_min_path=-1.0, voxel_p_lo=0.1, voxel_p_hi=99.9, zinger_abs=0.0).items():
        assert float.fromhex(got[name]) == (float(np.float32(value)) if name in F32 else value), name


@pytest.mark.parametrize("flag", sorted(OPTIONS))
def test_accepted_values_set_their_fields(answers, flag):
    for value, want in OPTIONS[flag][2]:
        assert_fields(answers[(flag, value)], want, (flag, value))


@pytest.mark.parametrize("flag", sorted(OPTIONS))
def test_refused_values_name_the_usage(answers, flag):
    usage, words, _, refused = OPTIONS[flag]
    for r in refused:
        value, said = (r, words) if isinstance(r, str) else r
        line = answers[(flag, value)]
        assert line.startswith("refused: " + usage) and said in line, (flag, value, line)
        if said == "cannot read":
            assert line == "refused: %s: cannot read '%s'" % (usage, value), (flag, value, line)


@pytest.mark.parametrize("name", sorted(OUT_OF_RANGE))
def test_out_of_range_text(answers, name):
    for flag, value, want in OUT_OF_RANGE[name]:
        assert_fields(answers[(flag, value)], want, (flag, value))


def test_a_flag_outside_the_table_is_not_looked_up(answers):
    assert answers[("--no-such-option", "1")] == "refused: unknown option --no-such-option"
