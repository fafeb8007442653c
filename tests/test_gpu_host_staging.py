"""The page-locked staging a handle owns (csrc/host_res.h: Pinned, Event, StagingRing) in its plain lifecycle on the MI355X: the
statistics ring of grl_set_obs_stats wrapping with no synchronisation in between, the grow-only staging of grl_act growing and
being reused, and handles created, used and destroyed one after the other in one process, half of them through a one-rank
exchange set-up.  Small vector shapes; every comparison is word for word."""
import numpy as np
import pytest

from grasp_rl import _capi
from grasp_rl.engine import QEngine, SacEngine

pytestmark = pytest.mark.gpu

OD, A, B, NA, CAP, LAYERS = 24, 4, 8, 3, 32, (16, 16)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sac_engine():
    cfg = _capi.make_config("mlp", obs_dim=OD, act_dim=A, layers=LAYERS, batch_size=B, act_batch=NA, replay_capacity=CAP, normalize=True)
    return with_params(SacEngine(cfg))


def q_engine():
    """layer-normalised: the launch-list route of the greedy act, which stages the observations through page-locked memory"""
    cfg = _capi.make_q_config("dqn", OD, 1, 3, common=(), branch_hidden=(16,), value_hidden=(16,), batch_size=B, act_batch=NA,
                              replay_capacity=CAP, normalize=True, layer_norm=True)
    return with_params(QEngine(cfg))


def with_params(eng):
    rng = np.random.default_rng(5)
    eng.be.write(eng.state[: eng.sizes.n_params], rng.uniform(-0.2, 0.2, eng.sizes.n_params).astype(np.float32))
    eng.be.synchronize()
    return eng


def stat_set(k):
    j = np.arange(OD)
    return 0.01 * (j + 1) * (k + 1), 0.5 + 0.125 * ((j + k) % 5), 1.0 + 0.5 * k


def raw_rows(n=NA):
    return (np.random.default_rng(9).normal(0.5, 2.0, (n, OD)) * (1.0 + np.arange(OD) % 3)).astype(np.float32)


def test_statistic_sets_back_to_back_leave_the_last_one():
    a, b = sac_engine(), sac_engine()
    for k in range(5):      # the ring of two mirrors wraps twice; nothing synchronises in between
        a.set_obs_stats(*stat_set(k))
    b.set_obs_stats(*stat_set(4))
    obs = raw_rows()
    got, want = a.act(obs, raw=True), b.act(obs, raw=True)
    assert np.isfinite(want).all() and np.array_equal(words(got), words(want))
    assert np.array_equal(words(a.be.to_host(a.state)), words(b.be.to_host(b.state)))
    a.close()
    b.close()


def test_act_staging_grows_and_is_reused(monkeypatch, capfd):
    obs = raw_rows()
    sac = sac_engine()
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    q = q_engine()
    assert "epsilon-greedy act: launch list of the Q-value path + select kernel" in capfd.readouterr().err
    for eng, act in ((sac, lambda x: sac.act(x)), (q, lambda x: q.act_bins(x)), (q, lambda x: q.q_values(x))):
        first, middle, third = act(obs[:1]), act(obs), act(obs[:1])
        assert np.isfinite(first.astype(np.float64)).all()
        assert np.array_equal(words(first), words(third)) and np.array_equal(words(first), words(middle[:1]))
    sac.close()
    q.close()


def test_handles_created_used_and_destroyed_in_turn():
    obs = raw_rows()
    results = []
    for k in range(20):
        eng = sac_engine()
        if k % 2:      # a one-rank exchange: set up, connected, released again
            eng.allreduce_connect([eng.allreduce_init(0, 1)])
            eng.allreduce_disconnect()
        eng.observe(obs)
        eng.set_obs_stats(*stat_set(2))
        results.append(eng.act(NA, raw=True, observed=True))
        eng.close()
    assert np.isfinite(results[0]).all()
    assert np.array_equal(words(results[-1]), words(results[0]))
