"""Which legs beside the headline a bench.py run takes on: none in a plain run, each at its old default with --full, and an
option given on the command line wins either way (no GPU needed)."""
import argparse

import bench


def _resolved(full, **given):
    args = argparse.Namespace(full=full, **{name: None for name in bench.FULL_LEGS})
    for name, value in given.items():
        setattr(args, name, value)
    return bench.resolve_legs(args)


def test_plain_run_leaves_every_leg_off_and_full_runs_them_at_their_defaults():
    plain, full = _resolved(False), _resolved(True)
    assert all(getattr(plain, name) == 0 for name in bench.FULL_LEGS)
    assert {name: getattr(full, name) for name in bench.FULL_LEGS} == {
        "live_traffic": 1, "noskip_step": 1, "fused_steps": 8, "cpu_budget": 15.0, "cpu_c1": 1, "workloads": 1, "paris_loop": 1}


def test_an_option_given_on_the_command_line_wins():
    assert _resolved(False, fused_steps=2).fused_steps == 2 and _resolved(False, fused_steps=2).noskip_step == 0
    assert _resolved(True, cpu_budget=0.0).cpu_budget == 0.0 and _resolved(True, cpu_budget=0.0).cpu_c1 == 1
