"""TRPO on the MI355X at the shapes where csrc/trpo_kernels.h / csrc/plan_trpo.inl change what they do BY SHAPE
(tests/trpo_util.py: SHAPE_CASES): one full block of the loss launch and a block with one live row, 64 action components, four
tangent levels with one action, the reducing vector launches at one workgroup, at two with an uneven split and at the cap of 256
(the 8192-value image observation: 1 081 741 entries, first layer in partial sums) -- rollout, GAE and one learn iteration against
the float64 restatement with the tolerance rule of tests/trpo_util.py, unchanged, the route and the workgroup count each case
exists for asserted from the plan dump."""
import pytest

import ppo_util as pu
import trpo_util as tu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(tu.SHAPE_CASES))
def test_update_and_route_at_shape_boundaries(name, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    c = tu.make_case(name)
    eng = tu.make_engine(c)
    plan = capfd.readouterr().err
    o64, m = tu.check_update(eng, c)
    eng.close()
    assert o64["ls_index"] >= 0 and o64["cg_iters"] == c["cg_iters"]
    assert o64["n_vf"] == 3 * (c["T"] // 128)
    assert tu.vec_blocks_from_dump(plan) == (tu.n_trainable(c), tu.SHAPE_CASES[name]["vec_blocks"])
    assert pu.route_from_dump(plan) == pu.declared_route(name, tu.SHAPE_CASES), plan


@pytest.mark.parametrize("name", list(tu.SHAPE_CASES))
def test_step_records_the_rollout_and_gae_follows_the_recursion(name):
    c = tu.make_case(name)
    eng = tu.make_engine(c)
    tu.check_step_and_gae(eng, c)
    eng.close()
