"""``PPO2(device_norm=True)`` / ``TRPO(device_norm=True)`` against the host path on the MI355X, both runs on the device engine:
everything the loop leaves behind, bit for bit (bodies: tests/ppo_norm_util.py; tests/test_ppo_norm_learn_host.py runs them on the
emulation build)."""
import pytest

import ppo_norm_util as nu
from grasp_rl.sb.ppo2 import PPO2

pytestmark = pytest.mark.gpu


@pytest.fixture
def clean(monkeypatch):
    for var in ("GRL_NUM_ENVS", "GRL_DEVICE_NORM", "GRL_TUNE"):
        monkeypatch.delenv(var, raising=False)


@pytest.mark.parametrize("algo,n", nu.LEARN_CASES)
def test_device_path_equals_host_path(clean, algo, n):
    nu.check_device_equals_host(algo, n)


def test_switches_and_auto(clean, monkeypatch):
    nu.check_switches(monkeypatch)


@pytest.mark.parametrize("algo,n", [("ppo2", 4), ("trpo", 1)])
def test_training_cleared_mid_run_falls_back_to_the_host(clean, algo, n):
    nu.check_frozen_mid_run(algo, n)


def test_loaded_without_env_warns_and_stays_on_the_host(clean, tmp_path, monkeypatch):
    nu.check_loaded_without_env(tmp_path, monkeypatch, PPO2.load)
