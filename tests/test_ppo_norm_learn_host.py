"""``PPO2(device_norm=True)`` / ``TRPO(device_norm=True)`` -- the VecNormalize observation statistics on the device while ``learn``
runs -- against the host path on the emulation build: everything the loop leaves behind, bit for bit (bodies: tests/
ppo_norm_util.py; tests/test_gpu_ppo_norm_learn.py runs them on the MI355X)."""
import pytest

import ppo_norm_util as nu
from grasp_rl.engine import PpoEngine, TrpoEngine
from grasp_rl.sb.ppo2 import PPO2
from grasp_rl.sb.trpo import TRPO
from hostemu_backend import NumpyHostBackend


@pytest.fixture
def emulated(monkeypatch, hostemu_lib):
    for var in ("GRL_NUM_ENVS", "GRL_DEVICE_NORM", "GRL_TUNE"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(PPO2, "_engine_factory", staticmethod(
        lambda cfg, ppo, device: PpoEngine(cfg, ppo, backend=NumpyHostBackend(), lib_path=hostemu_lib)))
    monkeypatch.setattr(TRPO, "_engine_factory", staticmethod(
        lambda cfg, trpo, device: TrpoEngine(cfg, trpo, backend=NumpyHostBackend(), lib_path=hostemu_lib)))


@pytest.mark.parametrize("algo,n", nu.LEARN_CASES)
def test_device_path_equals_host_path(emulated, algo, n):
    nu.check_device_equals_host(algo, n)


def test_switches_and_auto(emulated, monkeypatch):
    nu.check_switches(monkeypatch)


@pytest.mark.parametrize("algo,n", [("ppo2", 4), ("trpo", 1)])
def test_training_cleared_mid_run_falls_back_to_the_host(emulated, algo, n):
    nu.check_frozen_mid_run(algo, n)


def test_loaded_without_env_warns_and_stays_on_the_host(emulated, tmp_path, monkeypatch):
    nu.check_loaded_without_env(tmp_path, monkeypatch, PPO2.load)
