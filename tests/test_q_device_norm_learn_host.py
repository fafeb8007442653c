"""``DQN.learn`` / ``BDQ.learn`` with ``device_norm=True`` against ``device_norm=False`` over the emulation build (tests/
q_device_norm_learn_util.py): the host loop's decisions -- attach / detach, acting on the observed rows, replay_add_observed, no
statistics push -- and the resume of a checkpoint saved while the statistics were on the device."""
import pytest

import q_device_norm_learn_util as ql
from grasp_rl.engine import QEngine
from grasp_rl.sb.dqn import BDQ, DQN
from hostemu_backend import NumpyHostBackend


@pytest.fixture(autouse=True)
def emulation(hostemu_lib, monkeypatch):
    factory = staticmethod(lambda cfg, device: QEngine(cfg, backend=NumpyHostBackend(), lib_path=hostemu_lib))
    monkeypatch.setattr(DQN, "_engine_factory", factory, raising=False)
    monkeypatch.setattr(BDQ, "_engine_factory", factory, raising=False)
    monkeypatch.delenv("GRL_DEVICE_NORM", raising=False)


@pytest.mark.parametrize("algo,per,n", ql.CASES)
def test_learn_with_device_statistics_equals_host_statistics(algo, per, n):
    ql.check_device_equals_host(algo, per, n)


def test_checkpoint_saved_with_device_statistics_continues(tmp_path, monkeypatch):
    ql.check_checkpoint_continues("bdq", True, tmp_path, monkeypatch)


def test_unset_variable_means_off_for_q_models(monkeypatch):
    env = ql.make_env("bdq", 1)
    assert ql.make_model("bdq", env, False, None).device_norm is False
    for value, want in (("1", True), ("auto", "auto"), ("0", False)):
        monkeypatch.setenv("GRL_DEVICE_NORM", value)
        assert ql.make_model("bdq", ql.make_env("bdq", 1), False, None).device_norm == want
