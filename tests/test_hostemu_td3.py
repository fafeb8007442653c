"""TD3 through the C ABI on the g++ emulation build (the element kernels of csrc/td3_kernels.h as they stand, the loss kernel in its
sequential reference form, tests/hostemu/td3_kernels_ref1.h): layout, the update against the float64 restatement of
tests/td3_util.py over its case table, the policy delay, the shape of a call, device draws, and what a TD3 handle refuses."""
import ctypes as C
import os

import numpy as np
import pytest

import td3_util as tu
from grasp_rl import _capi
from hostemu_backend import NumpyHostBackend

NAMES = sorted(tu.CASES)


@pytest.fixture(scope="module")
def emu(hostemu_lib):
    os.environ.pop("GRL_TUNE", None)
    return hostemu_lib


def _make(lib):
    return lambda c, delay=2, seed=None: tu.make_engine(c, backend=NumpyHostBackend(), lib_path=lib, delay=delay, seed=seed)


def test_parameter_table_is_tf_creation_order(emu):
    c = tu.make_case("odd")
    eng = _make(emu)(c)
    shapes = tu.param_shapes(c["obs_dim"], c["A"], c["layers"])
    assert [n for n, *_ in eng.table] == list(shapes)
    assert list(shapes)[:8] == ["model/pi/fc0/kernel:0", "model/pi/fc0/bias:0", "model/pi/fc1/kernel:0", "model/pi/fc1/bias:0",
                                "model/pi/fc2/kernel:0", "model/pi/fc2/bias:0", "model/pi/dense/kernel:0", "model/pi/dense/bias:0"]
    assert list(shapes)[8] == "model/values_fn/qf1/fc0/kernel:0" and list(shapes)[14] == "model/values_fn/qf1/qf1/kernel:0"
    for name, _, numel, shape, trainable in eng.table:
        assert tuple(shape) == tuple(shapes[name]) and numel == int(np.prod(shapes[name])), name
        assert trainable == name.startswith("model/"), name
    assert _capi.GrlConfig.ae_kernel.offset == C.sizeof(_capi.GrlConfig) - 32      # grl_config itself did not grow
    eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_forward_values(emu, name):
    c = tu.make_case(name)
    runs = []
    for _ in range(2):
        eng = _make(emu)(c)
        runs.append(tu.check_forward(eng, c))
        eng.close()
    for k in runs[0]:      # the emulation build fetches the same bits as its own second run
        assert tu.same_bits(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("name", NAMES)
def test_gradients_of_a_policy_and_a_critic_only_update(emu, name):
    c = tu.make_case(name)
    eng = _make(emu)(c)
    tu.check_gradients(eng, c)
    eng.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("delay,first_step", tu.DELAY_RUNS)
def test_delay(emu, name, delay, first_step):
    tu.check_delay(_make(emu), tu.make_case(name), delay, first_step)


@pytest.mark.parametrize("name", NAMES)
def test_one_call_of_six_equals_six_calls(emu, name):
    c = tu.make_case(name)
    tu.check_one_call_equals_six(_make(emu), c)
    tu.check_one_call_equals_six(_make(emu), c, explicit=True)


def test_policy_loss_is_carried_without_a_fetch(emu):
    tu.check_policy_loss_is_carried_without_a_fetch(_make(emu), tu.make_case("two_blocks"))


def test_graph_updates_agree(emu):
    """GRL_TUNE graph_updates groups the updates of a call (the emulation build runs every group eagerly: the grouping loop
    itself); 1, 4 and 16 agree."""
    c = tu.make_case("default")
    outs = []
    for g in (1, 4, 16):
        os.environ["GRL_TUNE"] = "graph_updates=%d" % g
        try:
            outs.append(tu.check_one_call_equals_six(_make(emu), c))
        finally:
            os.environ.pop("GRL_TUNE", None)
    for s, m in outs[1:]:
        assert not tu.same_state(outs[0][0], s) and tu.same_bits(outs[0][1], m)


def test_device_draws(emu):
    """eps NULL, idx NULL: the same seed gives the same bits over two calls, another seed differs; one of the two NULL draws the
    other alone; the unclipped normals of a large batch have the moments of standard normals (five standard errors)."""
    c = tu.make_case("default")
    states = []
    for seed in (5, 5, 6):
        eng = _make(emu)(c, seed=seed)
        eng.train(3, first_step=0)
        eng.train(3, first_step=3)
        states.append((tu.state_of(eng), eng.fetch("td3_noise"), eng.fetch("idx_raw")))
        eng.close()
    assert not tu.same_state(states[0][0], states[1][0]) and tu.same_bits(states[0][1], states[1][1])
    assert tu.same_state(states[0][0], states[2][0]) and not tu.same_bits(states[0][1], states[2][1])
    # idx handed over, eps drawn -- and the other way round
    eng = _make(emu)(c, seed=5)
    eng.train(1, idx=c["idx"][:1], first_step=0)
    assert np.array_equal(eng.fetch("idx_raw", (2 * c["B"],)).view(np.int64), c["idx"][0])
    noise = eng.fetch("td3_noise", (c["B"], c["A"]))
    assert np.isfinite(noise).all() and noise.std() > 0.5 and not tu.same_bits(noise, c["eps"][0])
    eng.train(1, eps=c["eps"][1:2], first_step=1)
    assert tu.same_bits(eng.fetch("td3_noise", (c["B"], c["A"])), c["eps"][1])
    eng.close()
    # B = 4096, one layer
    cb = tu.make_case("default", B=4096, layers=(8,))
    eng = _make(emu)(cb, seed=3)
    eng.train(1, first_step=1)
    z = eng.fetch("td3_noise", (4096, 5)).astype(np.float64).reshape(-1)
    eng.close()
    n = z.size
    assert abs(z.mean()) <= 5.0 / np.sqrt(n) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n), (z.mean(), z.var())


def test_act_returns_the_policy_output(emu):
    for name in ("default", "width_300", "A_max"):      # one launch | the launch list (a width beyond 256) | 64 components
        c = tu.make_case(name)
        eng = _make(emu)(c)
        ref = tu.Ref(c["P"], c)
        obs = c["tr"]["obs"][:4]
        a = eng.act(obs)
        tu.close_fwd(a, ref.act(obs), "pi(obs) " + name)
        out = np.empty((2, c["A"]), np.float32)
        _capi.check(eng.lib, eng.lib.grl_act(eng.h, obs.ctypes.data, 2, 0, None, out.ctypes.data))      # not GRL_ACT_DETERMINISTIC, no eps
        assert tu.same_bits(out, a[:2])
        assert eng.lib.grl_act(eng.h, obs.ctypes.data, 5, 1, None, out.ctypes.data) == -1 and b"act_batch" in eng.lib.grl_last_error()
        eng.close()


def test_raw_observations_are_normalised_on_the_act_path(emu):
    c = tu.make_case("norm_1")
    eng = _make(emu)(c)
    st, obs = c["stats"], c["tr"]["obs"][:3]
    obs_n = np.clip((obs.astype(np.float64) - st["mean"]) / np.sqrt(st["var"] + 1e-8), -10.0, 10.0).astype(np.float32)
    assert tu.same_bits(eng.act(obs, raw=True), eng.act(obs_n))
    eng.close()


def test_learning_rate_and_reset_optimizer(emu):
    c = tu.make_case("default")
    eng = _make(emu)(c)
    eng.set_learning_rate(0.0)
    eng.train(2, c["idx"][:2], c["eps"][:2], first_step=0)
    P = eng.get_parameters()
    assert all(np.array_equal(P[n], c["P"][n]) for n in P if n.startswith("model/"))      # (tau moved the targets towards the unmoved model)
    assert eng.adam_steps() == (2, 1)
    eng.reset_optimizer()
    assert eng.adam_steps() == (0, 0) and not eng.fetch("adam_m").any() and not eng.fetch("adam_v").any()
    eng.close()


def test_wrong_handle_and_config_checks(emu):
    import ppo_util
    import parity_util
    from grasp_rl.engine import SacEngine, QEngine
    lib = _capi.load_library(emu)
    c = tu.make_case("odd")
    eng = _make(emu)(c)
    z = np.zeros(256, np.float32)
    p = z.ctypes.data
    h = eng.h
    calls = {
        "grl_train_step": lambda: lib.grl_train_step(h, 1, None, None),
        "grl_train_step_per": lambda: lib.grl_train_step_per(h, 1, 1.0, None),
        "grl_train_step_allreduce": lambda: lib.grl_train_step_allreduce(h, 1, None, None),
        "grl_compute_grads": lambda: lib.grl_compute_grads(h, None, None),
        "grl_compute_grads_staged": lambda: lib.grl_compute_grads_staged(h, 0, None, None),
        "grl_apply_grads": lambda: lib.grl_apply_grads(h, 1.0),
        "grl_get_metrics": lambda: lib.grl_get_metrics(h, C.byref(_capi.GrlMetrics())),
        "grl_observe": lambda: lib.grl_observe(h, p, 1, 0),
        "grl_replay_add_observed": lambda: lib.grl_replay_add_observed(h, p, p, p, 1, None, None, 0),
        "grl_q_update_target": lambda: lib.grl_q_update_target(h),
        "grl_encode": lambda: lib.grl_encode(h, p, 1, p),
        "grl_allreduce_init": lambda: lib.grl_allreduce_init(h, 0, 1, p),
        "grl_state_size": lambda: lib.grl_state_size(h, C.byref(C.c_size_t())),
        "grl_state_export": lambda: lib.grl_state_export(h, p, 16),
        "grl_replay_segments": lambda: lib.grl_replay_segments(h, 0, None),
    }
    before = tu.state_of(eng)
    for name, call in calls.items():
        assert call() == -3, name
        assert name.encode() in lib.grl_last_error() and b"TD3 handle" in lib.grl_last_error(), name
    for name, call in {"grl_ppo_train": lambda: lib.grl_ppo_train(h, p, 1), "grl_trpo_update": lambda: lib.grl_trpo_update(h, None, 0),
                       "grl_bc_end": lambda: lib.grl_bc_end(h), "grl_gail_end": lambda: lib.grl_gail_end(h),
                       "grl_ae_train_step": lambda: lib.grl_ae_train_step(h, p, 1)}.items():
        assert call() == -3, name
    assert not tu.same_state(before, tu.state_of(eng))
    eng.close()
    # grl_td3_train on the other kinds of handle
    pc = ppo_util.make_case("odd_towers")
    sac_case = parity_util.make_case(extractor="mlp", B=8, n_replay=16, obs_dim=12)
    q_cfg = _capi.make_q_config("dqn", 6, 2, 3, batch_size=4, replay_capacity=8)
    for other in (SacEngine(sac_case["cfg"], backend=NumpyHostBackend(), lib_path=emu), QEngine(q_cfg, backend=NumpyHostBackend(), lib_path=emu),
                  ppo_util.make_engine(pc, backend=NumpyHostBackend(), lib_path=emu)):
        assert lib.grl_td3_train(other.h, 1, None, None, 0) == -3 and b"TD3 handles" in lib.grl_last_error()
        assert lib.grl_td3_get_metrics(other.h, p, 256) == -3
        other.close()
    # configuration checks name the field
    s = _capi.GrlSizes()
    for field, value, word in (("policy_delay", 0, b"policy_delay"), ("target_policy_noise", -0.1, b"target_policy_noise"),
                               ("target_noise_clip", -1.0, b"target_noise_clip")):
        cfg, t = tu.engine_config(c)
        setattr(t, field, value)
        assert lib.grl_td3_query_sizes(C.byref(cfg), C.byref(t), C.byref(s)) == -1 and word in lib.grl_last_error(), field
    cfg, t = tu.engine_config(c)
    cfg.extractor = 2
    assert lib.grl_td3_query_sizes(C.byref(cfg), C.byref(t), C.byref(s)) == -1 and b"extractor" in lib.grl_last_error()
    cfg, t = tu.engine_config(c)
    assert lib.grl_query_sizes(C.byref(cfg), C.byref(s)) == -1 and b"grl_td3_create" in lib.grl_last_error()
    cfg.act_dim = tu.A_MAX + 1
    assert lib.grl_td3_query_sizes(C.byref(cfg), C.byref(t), C.byref(s)) == -1 and b"act_dim" in lib.grl_last_error()
    cfg, t = tu.engine_config(c)
    assert lib.grl_td3_query_sizes(C.byref(cfg), C.byref(t), C.byref(s)) == 0
    # the call's own arguments
    eng = _make(emu)(c)
    assert lib.grl_td3_train(eng.h, 0, None, None, 0) == -1 and lib.grl_td3_train(eng.h, _capi.TD3_MAX_UPDATES + 1, None, None, 0) == -1
    assert lib.grl_td3_train(eng.h, 1, None, None, -1) == -1 and b"first_step" in lib.grl_last_error()
    eng.close()
    cfg, t = tu.engine_config(c)
    empty = tu.Td3Engine(cfg, t, backend=NumpyHostBackend(), lib_path=emu)
    assert lib.grl_td3_train(empty.h, 1, None, None, 0) == -3 and b"empty" in lib.grl_last_error()
    empty.close()


def test_plan_line_counts_the_launches(emu, capfd):
    for name in ("default", "one_layer_A1", "depth_4"):
        c = tu.make_case(name)
        os.environ["GRL_PLAN_DUMP"] = "1"
        try:
            capfd.readouterr()
            _make(emu)(c, 2).close()
            err = capfd.readouterr().err
        finally:
            os.environ.pop("GRL_PLAN_DUMP", None)
        critic, policy, delay = tu.planned_launches(err)
        assert delay == 2 and policy > critic
        assert tu.launches_per_update(_make(emu), c) == (critic, policy)
