"""VecNormalize statistics and observe-once on DQN / BDQ handles on the MI355X (tests/q_device_norm_util.py): norm_update_kernel
on a Q handle against RunningMeanStd, the normalising instantiation of q_act_kernel (csrc/q_act.h) and the ingest launch of the
launch-list route against the plain greedy act on the host's normalize_obs, grl_replay_add_observed against grl_replay_add, and
updates on device-side statistics against pushed ones -- everything bit for bit."""
import pytest

import q_device_norm_util as qd
from grasp_rl.engine import QEngine

pytestmark = pytest.mark.gpu


def make_engine(cfg):
    return QEngine(cfg)


def test_statistics_equal_running_mean_std():
    qd.check_statistics(make_engine)


@pytest.mark.parametrize("net,obs_dim,fused", qd.ACT_CASES)
def test_act_on_raw_and_observed_rows_equals_act_on_normalized_rows(net, obs_dim, fused, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qd.check_act(make_engine, lambda: capfd.readouterr().err, net, obs_dim, fused)


@pytest.mark.parametrize("net", ["dqn", "bdq"])
def test_observed_replay_rows_equal_replay_add(net):
    qd.check_replay_rows(make_engine, net)


@pytest.mark.parametrize("net,obs_dim", [("dqn", 100), ("bdq", 100), ("bdq", 129)])
def test_updates_on_device_statistics_equal_pushed_statistics(net, obs_dim):
    qd.check_updates(make_engine, net, obs_dim)


def test_state_errors():
    qd.check_errors(make_engine)
