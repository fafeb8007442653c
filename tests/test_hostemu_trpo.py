"""TRPO through the C ABI on the g++ emulation build (the kernels of csrc/trpo_kernels.h over the sequential forms of
tests/hostemu/trpo_kernels_ref1.h): rollout and GAE, then one learn iteration -- advantage standardisation, losses, gradient,
one Fisher product, conjugate gradient, line search, value fit -- against the float64 restatement of tests/trpo_util.py at
every shape of its table, the named branches, and what a TRPO handle refuses."""
import ctypes as C
import os

import numpy as np
import pytest

import trpo_util as tu
from grasp_rl import _capi
from hostemu_backend import NumpyHostBackend


@pytest.fixture(scope="module")
def emu(hostemu_lib):
    os.environ.pop("GRL_TUNE", None)
    return hostemu_lib


def _engine(c, lib):
    return tu.make_engine(c, backend=NumpyHostBackend(), lib_path=lib)


def test_generic_create_names_the_trpo_calls_and_other_entry_points_refuse(emu):
    lib = _capi.load_library(emu)
    c = tu.make_case("odd")
    cfg, t = tu.engine_config(c)
    s = _capi.GrlSizes()
    assert lib.grl_query_sizes(C.byref(cfg), C.byref(s)) == -1 and b"grl_trpo_query_sizes" in lib.grl_last_error()
    assert lib.grl_trpo_query_sizes(C.byref(cfg), C.byref(t), C.byref(s)) == 0
    t.cg_iters = 65
    assert lib.grl_trpo_query_sizes(C.byref(cfg), C.byref(t), C.byref(s)) == -1 and b"cg_iters" in lib.grl_last_error()
    t.cg_iters, t.ls_steps = 10, 17
    assert lib.grl_trpo_query_sizes(C.byref(cfg), C.byref(t), C.byref(s)) == -1 and b"ls_steps" in lib.grl_last_error()
    t.ls_steps, cfg.act_batch = 10, 2
    assert lib.grl_trpo_query_sizes(C.byref(cfg), C.byref(t), C.byref(s)) == -1 and b"act_batch" in lib.grl_last_error()
    eng = _engine(c, emu)
    assert [n for n, *_ in eng.table] == tu.pu.param_names(c["pi"], c["vf"])
    size = C.c_size_t()
    for call in (lambda: lib.grl_state_size(eng.h, C.byref(size)), lambda: lib.grl_train_step(eng.h, 1, None, None),
                 lambda: lib.grl_ppo_train(eng.h, None, 1), lambda: lib.grl_replay_size(eng.h)):
        assert call() == -3, lib.grl_last_error()      # GRL_ERR_STATE
    with pytest.raises(_capi.GrlError, match="no finished rollout"):
        eng.update(c["vf_perm"])
    tu.place_and_finish(eng, c)
    bad = c["vf_perm"].copy()
    bad[1, 3] = bad[1, 4]
    with pytest.raises(_capi.GrlError, match="perm row 1 is no permutation"):
        eng.update(bad)
    eng.close()


@pytest.mark.parametrize("name", sorted(tu.CASES))
def test_step_records_the_rollout_and_gae_follows_the_recursion(emu, name):
    c = tu.make_case(name)
    eng = _engine(c, emu)
    tu.check_step_and_gae(eng, c)
    eng.close()


@pytest.mark.parametrize("name", sorted(tu.CASES))
def test_update_against_the_float64_restatement(emu, name):
    c = tu.make_case(name)
    eng = _engine(c, emu)
    o64, m = tu.check_update(eng, c)
    assert o64["ls_index"] >= 0 and o64["cg_iters"] == c["cg_iters"]
    assert o64["n_vf"] == 3 * (c["T"] // 128)      # floor(T / 128) minibatches per iteration, the tail dropped
    eng.close()


def test_both_line_search_outcomes_occur():
    ks = {}
    for name in ("odd", "default_400", "two_blocks"):
        c = tu.make_case(name)
        r = tu.Ref(c["P"], c)
        adv, ret = tu.pu.gae_np(c["rew"][None], c["vpred"][None], c["es"][None], np.zeros(1, np.float32), np.ones(1, np.float32), c["gamma"], c["lam"])
        ks[name] = r.update(c["obs"], c["act"], adv[0], ret[0], c["vf_perm"])["ls_index"]
    assert min(ks.values()) <= 1 and max(ks.values()) >= 2, ks      # accepted at once / after halvings


def test_one_trial_that_needs_a_halving_restores_theta(emu):
    c = tu.make_case("default_400", ls_steps=1)
    eng = _engine(c, emu)
    o64, m = tu.check_update(eng, c, expect=lambda o: o["ls_index"] == -1 or pytest.fail("the case accepts the full step"))
    assert m["ls_index"] == -1 and o64["n_vf"] == 9
    eng.close()


def test_equal_advantages_are_a_zero_gradient(emu):
    """gamma 0 and equal rewards with a placed vpred of zero: every advantage is the same number, atarg exactly 0."""
    c = tu.make_case("default_400", gamma=0.0)
    c["rew"] = np.full(c["T"], 0.5, np.float32)
    c["vpred"] = np.zeros(c["T"], np.float32)
    eng = _engine(c, emu)
    o64, m = tu.check_update(eng, c, expect=lambda o: o["ls_index"] == -2 or pytest.fail("the gradient is not zero"))
    assert m["ls_index"] == -2 and m["cg_iters"] == 0 and not eng.fetch("trpo_atarg").any()
    eng.close()


def test_heavy_damping_leaves_cg_early(emu):
    c = tu.make_case("odd", cg_damping=1e3)
    eng = _engine(c, emu)
    o64, m = tu.check_update(eng, c, expect=lambda o: o["cg_iters"] < c["cg_iters"] or pytest.fail("CG ran all its iterations"))
    assert m["cg_iters"] == o64["cg_iters"] < c["cg_iters"]
    eng.close()


def test_entropy_bonus(emu):
    c = tu.make_case("two_blocks", entcoeff=0.01)
    eng = _engine(c, emu)
    o64, m = tu.check_update(eng, c)
    assert m["entbonus"] != 0.0
    eng.close()


def test_two_handles_leave_the_same_bits(emu):
    c = tu.make_case("default_400")
    snaps = []
    for _ in range(2):
        eng = _engine(c, emu)
        for _ in range(2):
            tu.place_and_finish(eng, c)
            eng.update(c["vf_perm"])
        snaps.append(tu.snapshot(eng))
        eng.close()
    for a, b in zip(*snaps):
        assert np.array_equal(a, b)
