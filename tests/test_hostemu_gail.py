"""GAIL through the C ABI on the g++ emulation build (the kernels of csrc/gail_kernels.h, the loss launch over the sequential form
of tests/hostemu/gail_kernels_ref1.h, the GEMM launches over their reference loops): the discriminator's updates and its reward
pass against the float64 restatement of tests/gail_util.py at every case of its table, the exact properties of a session, and
what the entry points refuse."""
import os

import numpy as np
import pytest

import gail_util as gu
import trpo_util as tu
from grasp_rl import _capi
from hostemu_backend import NumpyHostBackend


@pytest.fixture(scope="module")
def emu(hostemu_lib):
    os.environ.pop("GRL_TUNE", None)
    return hostemu_lib


def _engine(c, lib):
    return tu.make_engine(c, backend=NumpyHostBackend(), lib_path=lib)


@pytest.mark.parametrize("name", sorted(gu.CASES))
def test_the_seed_of_every_case_passes_the_preconditions(name):
    gu.preconditions(gu.make_case(name))


@pytest.mark.parametrize("name", sorted(gu.CASES))
def test_updates_against_the_float64_restatement(emu, name, monkeypatch, capfd):
    c = gu.make_case(name)
    eng = _engine(c, emu)
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    capfd.readouterr()
    gu.check_updates(eng, c)
    routes = gu.routes_from_dump(capfd.readouterr().err)
    assert routes["rewards"][0] == 7 and routes["update"][0] == 14, routes
    assert (routes["update"][1] != "whole") == (name == "wide_obs") and (routes["rewards"][1] != "whole") == (name == "wide_obs"), routes
    eng.close()


@pytest.mark.parametrize("name", sorted(gu.CASES))
def test_rewards_pass_gae_and_the_trpo_update_behind_it(emu, name):
    c = gu.make_case(name)
    eng = _engine(c, emu)
    gu.check_rewards(eng, c, trpo_update=name == "odd_37")
    eng.close()


def test_the_update_reads_unclipped_actions(emu):
    c = gu.make_case("odd_37")
    eng = _engine(c, emu)
    gu.check_update_reads_unclipped_actions(eng, c)
    eng.close()


@pytest.mark.parametrize("name", ["odd_37", "two_blocks"])
def test_one_call_of_four_updates_equals_four_calls(emu, name):
    c = gu.make_case(name)
    gu.check_one_call_equals_single_calls(lambda: _engine(c, emu), c)


def test_a_second_session_starts_fresh(emu):
    c = gu.make_case("odd_37")
    eng = _engine(c, emu)
    gu.check_second_session_starts_fresh(eng, c)
    eng.close()


def test_state_rules_by_message_and_nothing_moves(emu):
    c = gu.make_case("odd_37")
    eng = _engine(c, emu)
    gu.check_state_rules(eng, c)
    eng.close()


def test_a_session_leaves_the_handle_its_state_and_its_plan(emu, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    c = gu.make_case("two_blocks")
    gu.check_session_leaves_the_handle_alone(lambda: _engine(c, emu), c, capfd)


def test_foreign_handles_refuse_by_name(emu):
    import bc_util
    import parity_util
    import ppo_util
    lib = _capi.load_library(emu)
    ppo = ppo_util.make_engine(ppo_util.make_case("default_64_64"), backend=NumpyHostBackend(), lib_path=emu)
    sac = parity_util.engine_setup(bc_util.make_case("mlp_b8"), backend=NumpyHostBackend(), lib_path=emu)
    gu.check_foreign_handles_refuse(lib, [ppo.h, sac.h])
    ppo.close()
    sac.close()
