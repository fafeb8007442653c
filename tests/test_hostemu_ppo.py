"""PPO2 through the C ABI on the g++ emulation build (every kernel of csrc/ppo_kernels.h in its sequential reference form,
tests/hostemu/ppo_kernels_ref1.h): layout, rollout bookkeeping, GAE bits, the update against the float64 restatement of
tests/ppo_util.py at every route of the launch plan, and what a PPO handle refuses."""
import ctypes as C
import os

import numpy as np
import pytest

import ppo_util as pu
from grasp_rl import _capi
from hostemu_backend import NumpyHostBackend


@pytest.fixture(scope="module")
def emu(hostemu_lib):
    os.environ.pop("GRL_TUNE", None)
    return hostemu_lib


def _engine(c, lib):
    return pu.make_engine(c, backend=NumpyHostBackend(), lib_path=lib)


def test_parameter_table_is_tf_creation_order(emu):
    c = pu.make_case("odd_towers")
    eng = _engine(c, emu)
    shapes = pu.param_shapes(c["obs_dim"], c["A"], *pu.tower_shapes(c))
    assert [n for n, *_ in eng.table] == list(shapes)
    assert [n for n in shapes][:8] == ["model/pi_fc0/w:0", "model/pi_fc0/b:0", "model/vf_fc0/w:0", "model/vf_fc0/b:0",
                                       "model/vf_fc1/w:0", "model/vf_fc1/b:0", "model/vf_fc2/w:0", "model/vf_fc2/b:0"]
    for name, _, numel, shape, trainable in eng.table:
        assert tuple(shape) == tuple(shapes[name]) and numel == int(np.prod(shapes[name])), name
        assert trainable == (not name.startswith("model/q/")), name
    assert eng.table[-3][0] == "model/pi/logstd:0" and tuple(eng.table[-3][3]) == (1, c["A"])
    eng.close()


def test_generic_create_names_the_ppo_calls(emu):
    lib = _capi.load_library(emu)
    cfg, ppo = pu.engine_config(pu.make_case("odd_towers"))
    s = _capi.GrlSizes()
    assert lib.grl_query_sizes(C.byref(cfg), C.byref(s)) == -1
    assert b"grl_ppo_query_sizes" in lib.grl_last_error() and b"grl_ppo_create" in lib.grl_last_error()
    assert lib.grl_ppo_query_sizes(C.byref(cfg), C.byref(ppo), C.byref(s)) == 0
    cfg.batch_size = 5                                      # 21 rows
    assert lib.grl_ppo_query_sizes(C.byref(cfg), C.byref(ppo), C.byref(s)) == -1 and b"divide" in lib.grl_last_error()
    cfg.batch_size, cfg.algo = 7, 5
    assert lib.grl_query_sizes(C.byref(cfg), C.byref(s)) == -1 and b"algo must be 0..4" in lib.grl_last_error()
    cfg.algo, cfg.q_bins = 4, 3
    assert lib.grl_ppo_query_sizes(C.byref(cfg), C.byref(ppo), C.byref(s)) == -1 and b"q_*" in lib.grl_last_error()
    assert _capi.GrlConfig.ae_kernel.offset == C.sizeof(_capi.GrlConfig) - 32      # grl_config itself did not grow


@pytest.mark.parametrize("name", ["odd_towers", "width_300"])
def test_step_records_the_rollout_and_gae_has_numpy_bits(emu, name):
    c = pu.make_case(name)
    eng = _engine(c, emu)
    pu.check_step_and_gae(eng, c)
    eng.close()


@pytest.mark.parametrize("name", sorted(pu.CASES))
def test_update_against_the_float64_restatement(emu, name):
    c = pu.make_case(name)
    eng = _engine(c, emu)
    pu.check_update(eng, c)
    eng.close()


def test_first_update_alone(emu):
    """One minibatch, one epoch: the gradients the first update leaves in the bucket and Adam's first step."""
    c = pu.make_case("default_64_64", noptepochs=1, nmb=1)
    eng = _engine(c, emu)
    adv, ret = pu.place_and_finish(eng, c)
    ref = pu.Ref(c["P"], c)
    (mb,) = list(pu.minibatches(c, adv, ret))
    o = ref.update(mb, c["lr"])
    assert o["margin"] > pu.MARGIN
    eng.train(c["perm"])
    pu.close_fwd(eng.fetch("ppo_mean", o["mean"].shape), o["mean"], "mean")
    pu.close_grads(eng.get_gradients(), o["grads"], "first update")
    pu.close_params(eng.get_parameters(), ref, c["lr"], 1)
    m1 = eng.fetch("adam_m")
    for name, off, numel, shape, tr in eng.table:
        if tr:
            assert np.allclose(m1[off:off + numel].reshape(shape), 0.1 * o["grads"][name], rtol=2e-3, atol=1e-9), name
    eng.close()


def test_act_and_learning_rate(emu):
    c = pu.make_case("odd_towers")
    eng = _engine(c, emu)
    ref = pu.Ref(c["P"], c)
    obs = c["obs"][:, 0]
    pu.close_fwd(eng.act(obs), ref.act(obs)[0], "deterministic action")
    pu.close_fwd(eng.act(obs[:2], deterministic=False, eps=c["eps"][:2, 0]), ref.act(obs[:2], c["eps"][:2, 0])[0], "sampled action")
    a1, a2 = eng.act(obs, deterministic=False), eng.act(obs, deterministic=False)      # device draws: a fresh one per call
    assert np.isfinite(a1).all() and not np.array_equal(a1, a2)
    with pytest.raises(_capi.GrlError, match="not defined on it"):
        _capi.check(eng.lib, eng.lib.grl_act(eng.h, obs.ctypes.data, 1, 2, None, np.empty(8, np.float32).ctypes.data))
    assert not eng.fetch("ppo_act").any()                    # grl_act records nothing
    # the step size of the next training call: 0 leaves every parameter where it was
    eng.set_learning_rate(0.0)
    pu.place_and_finish(eng, c)
    eng.train(c["perm"])
    P = eng.get_parameters()
    assert all(np.array_equal(P[n], c["P"][n]) for n in P)
    eng.close()


def test_train_checks_its_permutations(emu):
    c = pu.make_case("odd_towers")
    eng = _engine(c, emu)
    pu.place_and_finish(eng, c)
    bad = c["perm"].copy()
    bad[1, 3] = bad[1, 4]
    with pytest.raises(_capi.GrlError, match="perm row 1 is no permutation"):
        eng.train(bad)
    bad = c["perm"].copy()
    bad[0, 0] = 21
    with pytest.raises(_capi.GrlError, match="perm row 0"):
        eng.train(bad)
    eng.train(c["perm"])                                     # the refused calls moved nothing
    eng.close()


def test_other_algorithms_entry_points_are_refused(emu):
    c = pu.make_case("odd_towers")
    eng = _engine(c, emu)
    lib, h = eng.lib, eng.h
    z = np.zeros(64, np.float32)
    p = z.ctypes.data
    calls = {
        "grl_train_step": lambda: lib.grl_train_step(h, 1, None, None),
        "grl_train_step_per": lambda: lib.grl_train_step_per(h, 1, 1.0, None),
        "grl_train_step_allreduce": lambda: lib.grl_train_step_allreduce(h, 1, None, None),
        "grl_compute_grads": lambda: lib.grl_compute_grads(h, None, None),
        "grl_compute_grads_staged": lambda: lib.grl_compute_grads_staged(h, 0, None, None),
        "grl_apply_grads": lambda: lib.grl_apply_grads(h, 1.0),
        "grl_replay_add": lambda: lib.grl_replay_add(h, p, p, p, p, p, 1),
        "grl_replay_size": lambda: lib.grl_replay_size(h),
        "grl_observe": lambda: lib.grl_observe(h, p, 1, 0),
        "grl_norm_update": lambda: lib.grl_norm_update(h, p, 1),
        "grl_q_update_target": lambda: lib.grl_q_update_target(h),
        "grl_ae_train_step": lambda: lib.grl_ae_train_step(h, p, 1),
        "grl_encode": lambda: lib.grl_encode(h, p, 1, p),
        "grl_allreduce_init": lambda: lib.grl_allreduce_init(h, 0, 1, p),
        "grl_state_size": lambda: lib.grl_state_size(h, C.byref(C.c_size_t())),
        "grl_replay_segments": lambda: lib.grl_replay_segments(h, 0, None),
    }
    before = eng.get_parameters()
    for name, call in calls.items():
        assert call() == -3, name
        assert name.encode() in lib.grl_last_error() and b"PPO handle" in lib.grl_last_error(), name
    after = eng.get_parameters()
    assert all(np.array_equal(before[n], after[n]) for n in before)
    eng.close()


def test_plan_dump_names_the_act_route(emu, capfd):
    os.environ["GRL_PLAN_DUMP"] = "1"
    try:
        for name, tune, word in (("odd_towers", None, "one launch"), ("odd_towers", "ppo_act=0", "ppo_act=0"),
                                 ("width_300", None, "a width beyond 256"), ("wide_obs", None, "observation beyond 2048")):
            if tune:
                os.environ["GRL_TUNE"] = tune
            capfd.readouterr()
            _engine(pu.make_case(name), emu).close()
            os.environ.pop("GRL_TUNE", None)
            err = capfd.readouterr().err
            lines = [l for l in err.splitlines() if l.startswith("grl plan: ppo_act ")]
            assert lines and all(word in l for l in lines), (name, tune, lines)
    finally:
        os.environ.pop("GRL_PLAN_DUMP", None)
        os.environ.pop("GRL_TUNE", None)


def test_launch_list_and_one_launch_act_agree(emu):
    """GRL_TUNE ppo_act=0 forces the launch list: same actions, values and neglogps as the one-launch kernel."""
    c = pu.make_case("default_64_64")
    outs = []
    for tune in (None, "ppo_act=0"):
        if tune:
            os.environ["GRL_TUNE"] = tune
        try:
            eng = _engine(c, emu)
        finally:
            os.environ.pop("GRL_TUNE", None)
        outs.append(eng.step(c["obs"][:, 0], c["done"][:, 0], c["eps"][:, 0]))
        eng.close()
    for a, b in zip(*outs):
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6)
