"""TD3 on the MI355X through the C ABI: the kernels of csrc/td3_kernels.h inside the launch plan of csrc/plan_td3.inl against the
float64 restatement of tests/td3_util.py, over its case table (tests/test_hostemu_td3.py runs the same checks on the emulation
build): forward values, gradients of a policy and of a critic-only update, the policy delay, the shape of a call -- one call of n
updates, graph replay, the grouping of updates into graphs -- device draws, the act path and the plan's launch counts."""
import os

import numpy as np
import pytest

import td3_util as tu

pytestmark = pytest.mark.gpu

NAMES = sorted(tu.CASES)


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("GRL_TUNE", "GRL_NO_GRAPH", "GRL_PLAN_DUMP"):
        monkeypatch.delenv(k, raising=False)


def _make(c, delay=2, seed=None):
    return tu.make_engine(c, delay=delay, seed=seed)


@pytest.mark.parametrize("name", NAMES)
def test_forward_values(name):
    c = tu.make_case(name)
    eng = _make(c)
    tu.check_forward(eng, c)
    eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_gradients_of_a_policy_and_a_critic_only_update(name):
    c = tu.make_case(name)
    eng = _make(c)
    tu.check_gradients(eng, c)
    eng.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("delay,first_step", tu.DELAY_RUNS)
def test_delay(name, delay, first_step):
    tu.check_delay(_make, tu.make_case(name), delay, first_step)


@pytest.mark.parametrize("name", NAMES)
def test_one_call_of_six_equals_six_calls(name):
    c = tu.make_case(name)
    tu.check_one_call_equals_six(_make, c)
    tu.check_one_call_equals_six(_make, c, explicit=True)


def test_graph_replay_equals_eager_and_graph_updates_agree(monkeypatch):
    """Six updates on the device draws, twice (the second call replays the graphs the first captured): GRL_NO_GRAPH and
    graph_updates 1, 4 and 16 leave the same bits."""
    c = tu.make_case("default")
    outs = []
    for env in ({}, {"GRL_NO_GRAPH": "1"}, {"GRL_TUNE": "graph_updates=1"}, {"GRL_TUNE": "graph_updates=4"}, {"GRL_TUNE": "graph_updates=16"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = _make(c)
        eng.train(tu.N_UPDATES, first_step=1)
        m1 = eng.metrics()
        eng.train(tu.N_UPDATES, first_step=1 + tu.N_UPDATES)
        outs.append((tu.state_of(eng), m1, eng.metrics()))
        eng.close()
        for k in env:
            monkeypatch.delenv(k, raising=False)
    for s, m1, m2 in outs[1:]:
        assert not tu.same_state(outs[0][0], s), tu.same_state(outs[0][0], s)
        assert tu.same_bits(outs[0][1], m1) and tu.same_bits(outs[0][2], m2)


def test_policy_loss_is_carried_without_a_fetch():
    tu.check_policy_loss_is_carried_without_a_fetch(_make, tu.make_case("two_blocks"))


def test_device_draws():
    """eps NULL, idx NULL: the same seed gives the same bits over two calls, another seed differs; the unclipped normals of a
    B = 4096 one-layer handle have the moments of standard normals (five standard errors, as the SAC soak test holds chi-square)."""
    c = tu.make_case("default")
    states = []
    for seed in (5, 5, 6):
        eng = _make(c, seed=seed)
        eng.train(3, first_step=0)
        eng.train(3, first_step=3)
        states.append((tu.state_of(eng), eng.fetch("td3_noise"), eng.fetch("idx_raw")))
        eng.close()
    assert not tu.same_state(states[0][0], states[1][0]) and tu.same_bits(states[0][1], states[1][1]) and tu.same_bits(states[0][2], states[1][2])
    assert tu.same_state(states[0][0], states[2][0]) and not tu.same_bits(states[0][1], states[2][1])
    eng = _make(c, seed=5)
    eng.train(1, idx=c["idx"][:1], first_step=0)      # idx handed over, eps drawn
    assert np.array_equal(eng.fetch("idx_raw", (2 * c["B"],)).view(np.int64), c["idx"][0])
    noise = eng.fetch("td3_noise", (c["B"], c["A"]))
    assert np.isfinite(noise).all() and noise.std() > 0.5 and not tu.same_bits(noise, c["eps"][0])
    eng.train(1, eps=c["eps"][1:2], first_step=1)     # idx drawn, eps handed over
    assert tu.same_bits(eng.fetch("td3_noise", (c["B"], c["A"])), c["eps"][1])
    eng.close()
    cb = tu.make_case("default", B=4096, layers=(8,))
    eng = _make(cb, seed=3)
    eng.train(1, first_step=1)
    z = eng.fetch("td3_noise", (4096, 5)).astype(np.float64).reshape(-1)
    eng.close()
    n = z.size
    print("draws: n %d mean %.3e var - 1 %.3e" % (n, z.mean(), z.var() - 1.0))
    assert abs(z.mean()) <= 5.0 / np.sqrt(n) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)


def test_act_returns_the_policy_output():
    for name in ("default", "width_300", "A_max", "norm_1"):      # one launch | the launch list (a width beyond 256) | 64 components
        c = tu.make_case(name)
        eng = _make(c)
        ref = tu.Ref(c["P"], c)
        obs = c["tr"]["obs"][:4]
        if name == "norm_1":      # raw rows: VecNormalize applied on the device
            st = c["stats"]
            obs_n = np.clip((obs.astype(np.float64) - st["mean"]) / np.sqrt(st["var"] + 1e-8), -10.0, 10.0).astype(np.float32)
            assert tu.same_bits(eng.act(obs, raw=True), eng.act(obs_n))
            obs = obs_n
        tu.close_fwd(eng.act(obs), ref.act(obs), "pi(obs) " + name)
        tu.close_fwd(eng.act(obs[:1]), ref.act(obs[:1]), "pi(obs) of one row " + name)
        eng.close()


def test_plan_line_counts_the_launches(capfd):
    for name in ("default", "one_layer_A1", "depth_4"):
        c = tu.make_case(name)
        os.environ["GRL_PLAN_DUMP"] = "1"
        try:
            capfd.readouterr()
            _make(c).close()
            err = capfd.readouterr().err
        finally:
            os.environ.pop("GRL_PLAN_DUMP", None)
        critic, policy, delay = tu.planned_launches(err)
        assert delay == 2 and policy > critic
        assert tu.launches_per_update(_make, c) == (critic, policy)
