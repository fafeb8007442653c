"""GAIL on the MI355X through the C ABI: the kernels of csrc/gail_kernels.h inside the launch plan of csrc/plan_gail.inl against the
float64 restatement of tests/gail_util.py, at the cases of tests/test_hostemu_gail.py -- input width 16 after padding with an odd
hidden width and a constant column, batch 2 in four minibatches, two blocks of the loss launch with short expert batches, a
split-K first layer -- and the bits: one call against single calls, graph replay against eager launches, two sessions, the
handle's own state with and without a session, refused calls."""
import numpy as np
import pytest

import gail_util as gu
import trpo_util as tu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(gu.CASES))
def test_updates_against_the_float64_restatement(name, monkeypatch, capfd):
    c = gu.make_case(name)
    eng = tu.make_engine(c)
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    capfd.readouterr()
    gu.check_updates(eng, c)
    routes = gu.routes_from_dump(capfd.readouterr().err)
    assert routes["rewards"][0] == 7 and routes["update"][0] == 14, routes
    assert (routes["update"][1] != "whole") == (name == "wide_obs") and (routes["rewards"][1] != "whole") == (name == "wide_obs"), routes
    eng.close()


@pytest.mark.parametrize("name", sorted(gu.CASES))
def test_rewards_pass_gae_and_the_trpo_update_behind_it(name):
    c = gu.make_case(name)
    eng = tu.make_engine(c)
    gu.check_rewards(eng, c, trpo_update=name == "odd_37")
    eng.close()


def test_the_update_reads_unclipped_actions():
    c = gu.make_case("odd_37")
    eng = tu.make_engine(c)
    gu.check_update_reads_unclipped_actions(eng, c)
    eng.close()


@pytest.mark.parametrize("name", ["odd_37", "two_blocks", "wide_obs"])
def test_one_call_of_four_updates_equals_four_calls_and_graph_replay_equals_eager(name, monkeypatch):
    c = gu.make_case(name)
    graph = gu.check_one_call_equals_single_calls(lambda: tu.make_engine(c), c)
    monkeypatch.setenv("GRL_NO_GRAPH", "1")
    eager = gu.check_one_call_equals_single_calls(lambda: tu.make_engine(c), c)
    for a, b in zip(graph, eager):
        assert np.array_equal(a, b)


def test_a_second_session_starts_fresh():
    c = gu.make_case("odd_37")
    eng = tu.make_engine(c)
    gu.check_second_session_starts_fresh(eng, c)
    eng.close()


def test_state_rules_by_message_and_nothing_moves():
    c = gu.make_case("odd_37")
    eng = tu.make_engine(c)
    gu.check_state_rules(eng, c)
    eng.close()


def test_a_session_leaves_the_handle_its_state_and_its_plan(monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    c = gu.make_case("two_blocks")
    gu.check_session_leaves_the_handle_alone(lambda: tu.make_engine(c), c, capfd)
