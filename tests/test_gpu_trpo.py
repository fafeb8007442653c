"""TRPO on the MI355X through the C ABI: the kernels of csrc/trpo_kernels.h inside the launch plan of csrc/plan_trpo.inl against
the float64 restatement of tests/trpo_util.py, at the shapes of tests/test_hostemu_trpo.py -- towers that differ with T < 128,
the reference's 400-step batch, two blocks of the loss launch, an observation beyond 2048 values, a width beyond 256, T a
multiple of 5 and of 128 -- the named branches of the update, and the bits: two handles, and graph replay against eager launches."""
import numpy as np
import pytest

import trpo_util as tu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(tu.CASES))
def test_update_against_the_float64_restatement(name):
    c = tu.make_case(name)
    eng = tu.make_engine(c)
    o64, m = tu.check_update(eng, c)
    assert o64["ls_index"] >= 0 and o64["cg_iters"] == c["cg_iters"]
    assert o64["n_vf"] == 3 * (c["T"] // 128)
    eng.close()


@pytest.mark.parametrize("name", sorted(tu.CASES))
def test_step_records_the_rollout_and_gae_follows_the_recursion(name):
    c = tu.make_case(name)
    eng = tu.make_engine(c)
    tu.check_step_and_gae(eng, c)
    eng.close()


def test_one_trial_that_needs_a_halving_restores_theta():
    c = tu.make_case("default_400", ls_steps=1)
    eng = tu.make_engine(c)
    o64, m = tu.check_update(eng, c, expect=lambda o: o["ls_index"] == -1 or pytest.fail("the case accepts the full step"))
    assert m["ls_index"] == -1 and o64["n_vf"] == 9
    eng.close()


def test_equal_advantages_are_a_zero_gradient():
    c = tu.make_case("default_400", gamma=0.0)
    c["rew"] = np.full(c["T"], 0.5, np.float32)
    c["vpred"] = np.zeros(c["T"], np.float32)
    eng = tu.make_engine(c)
    o64, m = tu.check_update(eng, c, expect=lambda o: o["ls_index"] == -2 or pytest.fail("the gradient is not zero"))
    assert m["ls_index"] == -2 and m["cg_iters"] == 0 and not eng.fetch("trpo_atarg").any()
    eng.close()


def test_heavy_damping_leaves_cg_early():
    c = tu.make_case("odd", cg_damping=1e3)
    eng = tu.make_engine(c)
    o64, m = tu.check_update(eng, c, expect=lambda o: o["cg_iters"] < c["cg_iters"] or pytest.fail("CG ran all its iterations"))
    assert m["cg_iters"] == o64["cg_iters"] < c["cg_iters"]
    eng.close()


def test_entropy_bonus():
    c = tu.make_case("two_blocks", entcoeff=0.01)
    eng = tu.make_engine(c)
    o64, m = tu.check_update(eng, c)
    assert m["entbonus"] != 0.0
    eng.close()


def _two_updates(c):
    eng = tu.make_engine(c)
    for _ in range(2):      # the second call replays the graphs the first captured
        tu.place_and_finish(eng, c)
        eng.update(c["vf_perm"])
    snap = tu.snapshot(eng)
    eng.close()
    return snap


def test_two_handles_leave_the_same_bits():
    c = tu.make_case("default_400")
    for a, b in zip(_two_updates(c), _two_updates(c)):
        assert np.array_equal(a, b)


def test_graph_replay_equals_eager(monkeypatch):
    c = tu.make_case("two_blocks")
    replay = _two_updates(c)
    monkeypatch.setenv("GRL_NO_GRAPH", "1")
    eager = _two_updates(c)
    for a, b in zip(replay, eager):
        assert np.array_equal(a, b)
