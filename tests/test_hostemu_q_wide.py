"""Wide DQN / BDQ handles (tests/q_wide_util.py) on the CPU through the TEST-ONLY emulation build: the route (from GRL_PLAN_DUMP),
the tile table and the tiled clip + Adam launches in their sequential reference form (tests/hostemu/q_wide_ref1.h), the layer-0
partial sums, and every property of the wide route that does not need the device.  The kernels are tests/test_gpu_q_wide.py's."""
import os

import numpy as np
import pytest

import q_parity_util as qu
import q_wide_util as qw
from hostemu_backend import NumpyHostBackend

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_reference_conditions_hold_for_every_case():
    """on the reference alone: no sign-ambiguous hidden unit, clipping active / exactly off, act rows' top-two gap"""
    for name in qw.WIDE_CASES:
        case, s64 = qw.references(name)[:2]
        qw.assert_reference_conditions(case, s64)
        assert all(qw.act_gap_ok(case, n) for n in qw.ACT_NS), name


def test_131072_floats_is_not_wide_and_keeps_the_parent_plan(hostemu_lib, monkeypatch, capfd):
    """obs_dim 2048 x 64 == 131 072 floats: no q_wide line, the three-launch apply, an uncut q_l0 -- and the launch lines the dump
    equals, byte for byte, the one the parent's emulation build prints for this handle (tests/golden/)."""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    plan = qw.edge_plan(2048, lambda: capfd.readouterr().err, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    assert qw.wide_line(plan) is None and "q_wide" not in plan, plan
    assert "in one launch: no" in plan
    assert "q_sumsq" not in plan and "q_clip_adam" not in plan
    assert plan == open(os.path.join(GOLD, "q_plan_dump_obs2048_parent_emu.txt")).read(), plan       # the parent's emulation build


def test_131136_floats_is_the_first_wide_handle(hostemu_lib, monkeypatch, capfd):
    """obs_dim 2049 (ldf 2052) x 64: the q_wide line names both decisions; one update runs on the padded rows"""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    plan = qw.edge_plan(2049, lambda: capfd.readouterr().err, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    line = qw.wide_line(plan)
    assert line is not None, plan
    assert "q_sumsq + q_clip_adam" in line and "partial sums" in line, line
    n_tiles = 2 * ((2049 * 64 + qw.TILE - 1) // qw.TILE) + 2 + 2 + 6      # the two first kernels; 64 x 64, output kernels, biases
    assert "%d tiles" % n_tiles in line, (n_tiles, line)
    split = int(line.split("q_l0: ")[1].split()[0])
    assert 6 * split >= 64 and 6 * (split - 1) < 64, line          # six one-tile problems cut until the launch has 64 tiles


@pytest.mark.parametrize("name", qw.PARITY_CASES)
def test_wide_plan_matches_the_float64_reference(hostemu_lib, name, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qw.run_and_compare_wide(name, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    out = capfd.readouterr()
    print(out.out)
    line = qw.wide_line(out.err)
    assert line is not None, out.err[:2000]
    ln_case = bool(qw.WIDE_CASES[name].get("layer_norm"))
    assert ("q_l0: 1 partial" in line) == ln_case, line           # (layer norm: per-layer launches, no chain to add partial sums)


@pytest.mark.parametrize("name,n", [("dqn8192_B32", 1), ("dqn8192_B32", 16), ("dqn8192_B32", 17), ("bdq8192_B16", 17), ("dqn8192_ln", 16)])
def test_wide_act_bins_equal_the_argmax_of_the_reference(hostemu_lib, name, n):
    qw.act_check(name, n, backend=NumpyHostBackend(), lib_path=hostemu_lib)


@pytest.mark.parametrize("name", ["dqn8192_B50", "bdq8192_B16", "dqn8192_per", "dqn8192_ln"])
def test_one_call_of_n_updates_equals_n_calls(hostemu_lib, name):
    qw.multi_update_check(name, NumpyHostBackend, lib_path=hostemu_lib)


def test_checkpoint_and_continue_on_a_new_handle(hostemu_lib, tmp_path):
    qw.checkpoint_check("dqn8192_B32", NumpyHostBackend, str(tmp_path / "ck"), lib_path=hostemu_lib)
