"""The boundary shapes of tests/ppo_util.py (SHAPE_CASES) on the CPU through the TEST-ONLY emulation build: the table's declared
routes against a restatement of the routing conditions and against the plan the engine reports, and descriptors, arenas, rollout
bookkeeping and the update of every shape against the float64 restatement.  The emulation runs sequential loops where a workgroup
works together (tests/hostemu/ppo_kernels_ref1.h): the layer loop of ppo_act_kernel, the float4 paths of the tanh launches and
the wave / block sums are tests/test_gpu_ppo_shapes.py's.  `grid_stride` (a million activations per level) takes about a
second on the emulation build, so it runs here too."""
import os

import pytest

import ppo_util as pu
from hostemu_backend import NumpyHostBackend

EMU_CASES = list(pu.SHAPE_CASES)


@pytest.fixture(scope="module")
def emu(hostemu_lib):
    os.environ.pop("GRL_TUNE", None)
    return hostemu_lib


def _engine(c, lib):
    return pu.make_engine(c, backend=NumpyHostBackend(), lib_path=lib)


def test_declared_routes_follow_the_routing_conditions():
    for name in pu.SHAPE_CASES:
        a = pu.case_args(name)
        assert pu.planned_route(a["obs_dim"], tuple(a["pi"]) + tuple(a["vf"]), pu.first_layer_calls(a)) == pu.declared_route(name), name


def test_every_decision_has_a_case_on_each_side():
    routes = {n: pu.declared_route(n) for n in pu.SHAPE_CASES}
    for flag, yes, no in (("one", "act_in_2048", "in_2049_odd"), ("one", "width_256", "width_257"), ("list_obs", "in_2049_odd", "width_257"),
                          ("list_width", "width_257", "wide_quads"), ("split", "in_2049_odd", "act_in_2048"),
                          ("scalars", "in_2049_odd", "wide_quads"), ("quads", "wide_quads", "in_2049_odd"),
                          ("grid2", "grid_stride", "width_257")):
        assert flag in routes[yes] and flag not in routes[no], (flag, yes, no)
    # the row counts that are no route of the plan: blocks of the loss launch, of GAE, the 256-lane loops
    rows = {n: pu.SHAPE_CASES[n]["n_envs"] * pu.SHAPE_CASES[n]["n_steps"] // pu.SHAPE_CASES[n]["nmb"] for n in pu.SHAPE_CASES}
    assert (rows["mb_256"], rows["envs_257"], rows["mb_512"]) == (256, 257, 512)
    assert pu.SHAPE_CASES["envs_65"]["n_envs"] == 64 + 1 and pu.SHAPE_CASES["envs_257"]["n_envs"] == 256 + 1
    assert pu.SHAPE_CASES["A_64"]["A"] == 64 and len(pu.SHAPE_CASES["depth_4_1"]["pi"]) == 4


@pytest.mark.parametrize("name", EMU_CASES)
def test_update_and_route_at_shape_boundaries(emu, name, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    c = pu.make_case(name)
    eng = _engine(c, emu)
    plan = capfd.readouterr().err
    pu.check_update(eng, c)
    eng.close()
    assert pu.route_from_dump(plan) == pu.declared_route(name), plan


@pytest.mark.parametrize("name", pu.ACT_SHAPE_CASES)
def test_step_records_the_rollout_and_gae_has_numpy_bits(emu, name):
    c = pu.make_case(name)
    eng = _engine(c, emu)
    pu.check_step_and_gae(eng, c)
    eng.close()


@pytest.mark.parametrize("name", pu.ONE_LAUNCH_VS_LIST)
def test_launch_list_and_one_launch_act_agree(emu, name):
    pu.check_act_routes_agree(pu.make_case(name), lambda c: _engine(c, emu))


def test_device_draws_are_independent_standard_normals(emu):
    """(the draw is the header's own code in both builds; a second on the emulation build)"""
    pu.check_device_draws(lambda c: _engine(c, emu))
