"""VecNormalize statistics and observe-once on DQN / BDQ handles (tests/q_device_norm_util.py) on the CPU through the TEST-ONLY
emulation build: arenas, staging, the four act variants of both routes, ring bookkeeping, state errors.  The emulation runs
sequential reference loops in place of the kernels (tests/hostemu/q_act_ref2.h for the normalising act); the kernels themselves
are tests/test_gpu_q_device_norm.py's."""
import pytest

import q_device_norm_util as qd
from grasp_rl.engine import QEngine
from hostemu_backend import NumpyHostBackend


@pytest.fixture
def make_engine(hostemu_lib):
    return lambda cfg: QEngine(cfg, backend=NumpyHostBackend(), lib_path=hostemu_lib)


def test_statistics_equal_running_mean_std(make_engine):
    qd.check_statistics(make_engine)


@pytest.mark.parametrize("net,obs_dim,fused", qd.ACT_CASES)
def test_act_on_raw_and_observed_rows_equals_act_on_normalized_rows(make_engine, net, obs_dim, fused, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qd.check_act(make_engine, lambda: capfd.readouterr().err, net, obs_dim, fused)


@pytest.mark.parametrize("net", ["dqn", "bdq"])
def test_observed_replay_rows_equal_replay_add(make_engine, net):
    qd.check_replay_rows(make_engine, net)


@pytest.mark.parametrize("net,obs_dim", [("dqn", 100), ("bdq", 100), ("bdq", 129)])
def test_updates_on_device_statistics_equal_pushed_statistics(make_engine, net, obs_dim):
    qd.check_updates(make_engine, net, obs_dim)


def test_state_errors(make_engine):
    qd.check_errors(make_engine)
