"""The boundary shapes of tests/trpo_util.py (SHAPE_CASES) on the CPU through the TEST-ONLY emulation build: declared routes and
vector-launch workgroup counts against a restatement of the conditions and against the plan the engine reports; rollout, GAE and one
learn iteration of every shape against the float64 restatement.  The vector kernels (trpo_range over the emulated grid) are the
product's own code here; the loss launch and the block sums run in their sequential forms (tests/hostemu/trpo_kernels_ref1.h) and
are tests/test_gpu_trpo_shapes.py's."""
import os

import pytest

import ppo_util as pu
import trpo_util as tu
from hostemu_backend import NumpyHostBackend


@pytest.fixture(scope="module")
def emu(hostemu_lib):
    os.environ.pop("GRL_TUNE", None)
    return hostemu_lib


def _engine(c, lib):
    return tu.make_engine(c, backend=NumpyHostBackend(), lib_path=lib)


def test_declarations_follow_the_conditions_in_the_sources():
    for name, a in tu.SHAPE_CASES.items():
        assert tu.planned_vec_blocks(a) == a["vec_blocks"], name
        assert pu.planned_route(a["obs_dim"], tuple(a["pi"]) + tuple(a["vf"]), tu.first_layer_calls(a)) == pu.declared_route(name, tu.SHAPE_CASES), name
    entries = {name: tu.n_trainable(a, padded=False) for name, a in tu.SHAPE_CASES.items()}
    assert entries["T_256"] == 357 and entries["vec_4351"] == 4351 and entries["vec_8831"] == 8831 and entries["obs_8192"] == 1081741
    n = {name: tu.n_trainable(a) for name, a in tu.SHAPE_CASES.items()}      # what the vector launches run over
    assert n["T_256"] == 364 and n["vec_4351"] == 4356 and n["vec_8831"] == 8840 and n["obs_8192"] == 1081748
    assert max(v for v in n.values() if v <= 4096) == 4096 < n["bucket_4100"] < n["vec_4351"] < 2 * 4096 < n["vec_8831"] < 3 * 4096
    assert (n["bucket_4096"], n["bucket_4100"]) == (4096, 4100)
    assert n["vec_8831"] % 3                                                              # an uneven split
    per = -(-n["obs_8192"] // 256)
    assert n["obs_8192"] > 256 * 4096 and 255 * per < n["obs_8192"] < 256 * per           # the cap, a short last range
    T = {name: a["T"] for name, a in tu.SHAPE_CASES.items()}
    assert (T["T_256"], T["T_257"]) == (256, 257) and T["obs_8192"] < 128
    assert tu.SHAPE_CASES["A_64"]["A"] == 64 and len(tu.SHAPE_CASES["A_1_depth_4"]["pi"]) == 4


@pytest.mark.parametrize("name", list(tu.SHAPE_CASES))
def test_update_and_route_at_shape_boundaries(emu, name, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    c = tu.make_case(name)
    eng = _engine(c, emu)
    plan = capfd.readouterr().err
    o64, m = tu.check_update(eng, c)
    eng.close()
    assert o64["ls_index"] >= 0 and o64["cg_iters"] == c["cg_iters"]
    assert o64["n_vf"] == 3 * (c["T"] // 128)
    assert tu.vec_blocks_from_dump(plan) == (tu.n_trainable(c), tu.SHAPE_CASES[name]["vec_blocks"])
    assert pu.route_from_dump(plan) == pu.declared_route(name, tu.SHAPE_CASES), plan


@pytest.mark.parametrize("name", list(tu.SHAPE_CASES))
def test_step_records_the_rollout_and_gae_follows_the_recursion(emu, name):
    c = tu.make_case(name)
    eng = _engine(c, emu)
    tu.check_step_and_gae(eng, c)
    eng.close()
