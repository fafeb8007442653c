"""PPO2 on the MI355X through the C ABI: the kernels of csrc/ppo_kernels.h inside the launch plan of csrc/plan_ppo.inl against
the float64 restatement of tests/ppo_util.py, at the shapes of tests/test_hostemu_ppo.py -- the reference's default towers, towers
that differ, two blocks of the loss launch, an observation beyond 2048 values (first layer in partial sums, launch list), a width
beyond 256, no value clipping and no gradient clipping -- with GAE held to the bits of the NumPy float32 restatement."""
import numpy as np
import pytest

import ppo_util as pu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(pu.CASES))
def test_update_against_the_float64_restatement(name):
    c = pu.make_case(name)
    eng = pu.make_engine(c)
    pu.check_update(eng, c)
    eng.close()


@pytest.mark.parametrize("name", ["odd_towers", "width_300", "wide_obs"])
def test_step_records_the_rollout_and_gae_has_numpy_bits(name):
    c = pu.make_case(name)
    eng = pu.make_engine(c)
    pu.check_step_and_gae(eng, c)
    eng.close()


def test_launch_list_and_one_launch_act_agree(monkeypatch, capfd):
    """GRL_TUNE ppo_act=0 forces the launch list: the same actions, values and neglogps as ppo_act_kernel; the plan dump names
    the route each handle takes."""
    c = pu.make_case("default_64_64")
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    outs = []
    for tune, word in ((None, "one launch"), ("ppo_act=0", "launch list (ppo_act=0)")):
        if tune:
            monkeypatch.setenv("GRL_TUNE", tune)
        capfd.readouterr()
        eng = pu.make_engine(c)
        monkeypatch.delenv("GRL_TUNE", raising=False)
        lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("grl plan: ppo_act ")]
        assert lines and all(word in l for l in lines), lines
        outs.append(eng.step(c["obs"][:, 0], c["done"][:, 0], c["eps"][:, 0]))
        eng.close()
    for a, b in zip(*outs):
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_graph_replay_equals_eager(monkeypatch):
    """The updates of a training call replayed as captured graphs leave the bits the same launches leave run one by one."""
    c = pu.make_case("default_64_64")
    P = []
    for no_graph in (False, True):
        if no_graph:
            monkeypatch.setenv("GRL_NO_GRAPH", "1")
        eng = pu.make_engine(c)
        monkeypatch.delenv("GRL_NO_GRAPH", raising=False)
        for _ in range(2):      # the second call replays the graphs the first captured, from a reset cursor
            pu.place_and_finish(eng, c)
            eng.train(c["perm"])
        P.append((eng.get_parameters(), eng.metrics()))
        eng.close()
    for n in P[0][0]:
        assert np.array_equal(P[0][0][n], P[1][0][n]), n
    assert np.array_equal(P[0][1], P[1][1])


def test_device_draws_are_seeded_and_fresh():
    c = pu.make_case("odd_towers")
    a = []
    for _ in range(2):
        eng = pu.make_engine(c)
        a.append([eng.act(c["obs"][:, 0], deterministic=False) for _ in range(2)])
        mean = eng.act(c["obs"][:, 0])
        eng.close()
    assert np.array_equal(a[0][0], a[1][0]) and np.array_equal(a[0][1], a[1][1])      # same seed, same stream
    assert not np.array_equal(a[0][0], a[0][1]) and np.isfinite(a[0][0]).all()
    std = np.exp(c["P"]["model/pi/logstd:0"][0])
    assert (np.abs(a[0][0] - mean) < 6.0 * std).all()
