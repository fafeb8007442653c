"""Behaviour-cloning pretraining through the C ABI on the g++ emulation build (the kernels of csrc/bc_kernels.h over the
sequential form of tests/hostemu/bc_kernels_ref1.h, the GEMM launches over their reference loops): one update of every case of
tests/bc_util.py against the float64 restatement, the exact properties of a session, and what the entry points refuse."""
import ctypes as C
import os

import numpy as np
import pytest

import bc_util as bu
import parity_util as pu
from grasp_rl import _capi
from hostemu_backend import NumpyHostBackend


@pytest.fixture(scope="module")
def emu(hostemu_lib):
    os.environ.pop("GRL_TUNE", None)
    return hostemu_lib


def _engine(case, lib):
    return pu.engine_setup(case, backend=NumpyHostBackend(), lib_path=lib)


@pytest.mark.parametrize("name", sorted(bu.CASES))
def test_the_seed_of_every_case_keeps_relu_units_off_zero(name):
    bu.assert_no_sign_ambiguity(bu.make_case(name))


@pytest.mark.parametrize("name", sorted(bu.CASES))
def test_update_against_the_float64_restatement(emu, name, monkeypatch, capfd):
    case = bu.make_case(name)
    eng = _engine(case, emu)
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    capfd.readouterr()
    bu.check_update(eng, case)
    line = bu.route_from_dump(capfd.readouterr().err)
    assert "per-layer:" in line and "bc_batch %d " % case["bc_batch"] in line, line
    eng.close()


def test_per_layer_convolutions_match_too(emu, monkeypatch):
    monkeypatch.setenv("GRL_TUNE", "conv_stack=0")
    case = bu.make_case("depth_augmented")
    eng = _engine(case, emu)
    bu.check_update(eng, case)
    eng.close()


def test_adam_epsilon_is_the_sessions_own(emu):
    """the same data at adam_epsilon 1e-3 and 1e-8: each matches its own restatement (check_update), and they differ"""
    out = []
    for eps in (1e-3, 1e-8):
        case = bu.make_case("mlp_b8", adam_eps=eps)
        eng = _engine(case, emu)
        out.append(bu.check_update(eng, case))
        eng.close()
    assert any(not np.array_equal(out[0][n], out[1][n]) for n in bu.trained_names(case["spec"]))


@pytest.mark.parametrize("name", ["mlp_b17_tail3", "depth_augmented"])
def test_one_call_of_three_updates_equals_three_calls(emu, name):
    case = bu.make_case(name)
    bu.check_one_call_equals_single_calls(lambda: _engine(case, emu), case)


def test_a_second_session_starts_from_zero_moments(emu):
    case = bu.make_case("mlp_b8")
    bu.check_second_session_starts_fresh(lambda: _engine(case, emu), case)


@pytest.mark.parametrize("name", ["mlp_b32", "depth_augmented"])
def test_sac_updates_after_bc_equal_those_after_set_parameters(emu, name):
    case = bu.make_case(name)
    bu.check_pretrain_then_train_equals_set_parameters_then_train(lambda: _engine(case, emu), case)


def test_refused_calls_move_nothing(emu):
    case = bu.make_case("mlp_b17_tail3")
    eng = _engine(case, emu)
    bu.check_refusals_move_nothing(eng, case)
    eng.close()


def test_foreign_handles_refuse_by_name(emu):
    import ppo_util
    import q_parity_util as qu
    lib = _capi.load_library(emu)
    c = ppo_util.make_case("default_64_64")
    ppo = ppo_util.make_engine(c, backend=NumpyHostBackend(), lib_path=emu)
    q = qu.q_engine_setup(qu.make_q_case(**qu.CASES[sorted(qu.CASES)[0]]), backend=NumpyHostBackend(), lib_path=emu)
    n = C.c_size_t()
    for eng in (ppo, q):
        for call, what in ((lambda: lib.grl_bc_query_sizes(eng.h, None, C.byref(n)), b"grl_bc_query_sizes"),
                           (lambda: lib.grl_bc_begin(eng.h, None, None), b"grl_bc_begin"),
                           (lambda: lib.grl_bc_train(eng.h, None, None, 0, None, 1), b"grl_bc_train"),
                           (lambda: lib.grl_bc_eval(eng.h, None, None, 0, None, 1), b"grl_bc_eval"),
                           (lambda: lib.grl_bc_get_losses(eng.h, None, 0), b"grl_bc_get_losses"),
                           (lambda: lib.grl_bc_end(eng.h), b"grl_bc_end")):
            assert call() == -3                                     # GRL_ERR_STATE
            assert lib.grl_last_error() == what + b" is defined for SAC handles (grl_create)"
        eng.close()
