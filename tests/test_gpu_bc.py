"""Behaviour-cloning pretraining on the MI355X through the C ABI: the kernels of csrc/bc_kernels.h inside the launch plan of
csrc/plan_bc.inl against the float64 restatement of tests/bc_util.py, at the cases of tests/test_hostemu_bc.py -- a minibatch
below one 16-row block, a block plus one row with three absent rows, narrow, wide and single hidden layers, the three image
extractors, an asymmetric action space, two Adam epsilons -- and the bits: one call against single calls (graph replay against
single launches of the same list), two sessions, SAC updates behind a pretraining, refused calls."""
import numpy as np
import pytest

import bc_util as bu
import parity_util as pu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(bu.CASES))
def test_update_against_the_float64_restatement(name, monkeypatch, capfd):
    case = bu.make_case(name)
    eng = pu.engine_setup(case)
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    capfd.readouterr()
    bu.check_update(eng, case)
    line = bu.route_from_dump(capfd.readouterr().err)
    assert "per-layer:" in line and "bc_batch %d " % case["bc_batch"] in line, line
    eng.close()


def test_per_layer_convolutions_match_too(monkeypatch):
    monkeypatch.setenv("GRL_TUNE", "conv_stack=0")
    case = bu.make_case("depth_augmented")
    eng = pu.engine_setup(case)
    bu.check_update(eng, case)
    eng.close()


def test_adam_epsilon_is_the_sessions_own():
    out = []
    for eps in (1e-3, 1e-8):
        case = bu.make_case("mlp_b8", adam_eps=eps)
        eng = pu.engine_setup(case)
        out.append(bu.check_update(eng, case))
        eng.close()
    assert any(not np.array_equal(out[0][n], out[1][n]) for n in bu.trained_names(case["spec"]))


@pytest.mark.parametrize("name", ["mlp_b17_tail3", "depth_augmented"])
def test_one_call_of_three_updates_equals_three_calls(name):
    case = bu.make_case(name)
    bu.check_one_call_equals_single_calls(lambda: pu.engine_setup(case), case)


def test_a_second_session_starts_from_zero_moments():
    case = bu.make_case("mlp_b8")
    bu.check_second_session_starts_fresh(lambda: pu.engine_setup(case), case)


@pytest.mark.parametrize("name", ["mlp_b32", "depth_augmented"])
def test_sac_updates_after_bc_equal_those_after_set_parameters(name):
    case = bu.make_case(name)
    bu.check_pretrain_then_train_equals_set_parameters_then_train(lambda: pu.engine_setup(case), case)


def test_refused_calls_move_nothing():
    case = bu.make_case("mlp_b17_tail3")
    eng = pu.engine_setup(case)
    bu.check_refusals_move_nothing(eng, case)
    eng.close()
