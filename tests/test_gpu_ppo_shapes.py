"""PPO2 on the MI355X at the shapes where csrc/plan_ppo.inl and csrc/ppo_kernels.h change what they do BY SHAPE
(tests/ppo_util.py: SHAPE_CASES -- on the edges of every such decision, the smallest shapes that cross them): the limits of
ppo_act_kernel (2048 inputs, width 256, four layers), tanh_fwd over the partial sums of a split first layer without quads and with
quads that straddle rows, the grid-stride loops of the tanh launches, 64 action components in the loss, the gather and the sample
tail, full and one-row blocks of the loss launch, two GAE workgroups, the rewards loop's second pass -- against the float64
restatement with the tolerances of tests/ppo_util.py, unchanged, and with the route each case exists for asserted from the plan
dump.  Then the device draws behind grl_act against the statistics of independent standard normals."""
import pytest

import ppo_util as pu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(pu.SHAPE_CASES))
def test_update_and_route_at_shape_boundaries(name, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    c = pu.make_case(name)
    eng = pu.make_engine(c)
    plan = capfd.readouterr().err
    pu.check_update(eng, c)
    eng.close()
    assert pu.route_from_dump(plan) == pu.declared_route(name), plan


@pytest.mark.parametrize("name", pu.ACT_SHAPE_CASES)
def test_step_records_the_rollout_and_gae_has_numpy_bits(name):
    c = pu.make_case(name)
    eng = pu.make_engine(c)
    pu.check_step_and_gae(eng, c)
    eng.close()


@pytest.mark.parametrize("name", pu.ONE_LAUNCH_VS_LIST)
def test_launch_list_and_one_launch_act_agree(name, monkeypatch):
    monkeypatch.delenv("GRL_TUNE", raising=False)
    pu.check_act_routes_agree(pu.make_case(name), pu.make_engine)


def test_device_draws_are_independent_standard_normals():
    pu.check_device_draws(pu.make_engine)
