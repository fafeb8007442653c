"""The reference's own ``SBPolicy(..., algo="PPO").learn()`` (manipulation_main/training/sb_helper.py:137-154: ``sb.PPO2(
MlpPolicy, env, verbose=2, gamma=..., learning_rate=..., tensorboard_log=...)``) as ``train_stable_baselines.py train --config
config/gripper_grasp.yaml --algo PPO`` reaches it -- the image env, whose 64 x 64 x 2 observation the MlpPolicy takes flattened --
and on vector observations with tensorboard on: imported from where it lies, unmodified, on top of the alias package, the
emulation build and tests/fake_env.py -- the set-up of tests/test_reference_driver.py.  Skipped where /root/reference does not
exist (the GPU box)."""
import importlib
import os
import sys
import types

import numpy as np
import pytest

import stable_baselines as sb
from fake_env import FakeGraspEnv
from grasp_rl.engine import PpoEngine
from grasp_rl.sb import spaces
from grasp_rl.sb.ppo2 import PPO2
from hostemu_backend import NumpyHostBackend
from stable_baselines.bench import Monitor
from stable_baselines.common.vec_env import DummyVecEnv

REF_TRAINING = "/root/reference/manipulation_main/training"
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF_TRAINING, "sb_helper.py")),
                                reason="/root/reference is not present on this box")


@pytest.fixture
def reference_sb_helper(monkeypatch, hostemu_lib):
    tf = types.ModuleType("tensorflow")
    tf.nn = types.SimpleNamespace(relu=lambda x: x)
    tf.contrib = types.SimpleNamespace()
    tf.Summary = type("Summary", (), {"Value": staticmethod(lambda **k: k), "__init__": lambda self, **k: self.__dict__.update(k)})
    gym = types.ModuleType("gym")
    gym.Env = type("Env", (), {})
    gym.spaces = spaces
    monkeypatch.setitem(sys.modules, "tensorflow", tf)
    monkeypatch.setitem(sys.modules, "gym", gym)
    monkeypatch.syspath_prepend(REF_TRAINING)
    monkeypatch.delenv("GRL_NUM_ENVS", raising=False)
    for name in ("sb_helper", "base_callbacks", "custom_obs_policy"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    monkeypatch.setattr(PPO2, "_engine_factory", staticmethod(
        lambda cfg, ppo, device: PpoEngine(cfg, ppo, backend=NumpyHostBackend(), lib_path=hostemu_lib)))
    mod = importlib.import_module("sb_helper")
    assert os.path.realpath(mod.__file__).startswith("/root/reference/")
    yield mod
    for name in ("sb_helper", "base_callbacks", "custom_obs_policy"):
        sys.modules.pop(name, None)


def test_reference_sbpolicy_ppo_on_the_image_env(reference_sb_helper, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("models/ppo_img")
    config = {"normalize": False, "discount_factor": 0.99,
              "PPO": {"tensorboard_logs": None, "learning_rate": 0.001, "layers": [64, 64], "total_timesteps": "256"}}
    mk = lambda s: FakeGraspEnv("depth", seed=s)
    env = DummyVecEnv([lambda: Monitor(mk(0), os.path.join("models/ppo_img", "log_file"))])
    driver = reference_sb_helper.SBPolicy(env, DummyVecEnv([lambda: mk(1)]), config, "models/ppo_img", algo="PPO")
    driver.learn()                                            # two rollouts of 128 steps, 4 x 4 updates each
    assert os.path.isfile("models/ppo_img/ppo_img.zip")
    model = sb.PPO2.load("models/ppo_img/ppo_img.zip")        # train_stable_baselines.py:99-100
    assert tuple(model.observation_space.shape) == (64, 64, 2) and model.gamma == 0.99 and model.learning_rate == 0.001
    P = model.get_parameters()
    assert P["model/pi_fc0/w:0"].shape == (8192, 64) and P["model/pi/logstd:0"].shape == (1, 5)
    assert all(np.isfinite(v).all() for v in P.values()) and P["model/pi/logstd:0"].any()
    a, _ = model.predict(mk(2).reset(), deterministic=True)
    assert a.shape == (5,) and (np.abs(a) <= 1).all()


def test_reference_sbpolicy_ppo_with_tensorboard_and_normalize(reference_sb_helper, tmp_path, monkeypatch):
    """Vector observations, tensorboard on (TensorboardCallback writes through locals['writer']), and `normalize: True`: the PPO
    branch does not wrap the training env, so SBPolicy.save fails on None.save AFTER the zip is written -- as on stable-baselines."""
    monkeypatch.chdir(tmp_path)
    os.makedirs("models/ppo_vec")
    config = {"normalize": True, "discount_factor": 0.95,
              "PPO": {"tensorboard_logs": "yes", "learning_rate": 0.0003, "layers": [64, 64], "total_timesteps": 128}}
    mk = lambda s: FakeGraspEnv(vector_dim=101, seed=s, act_dim=3)
    env = DummyVecEnv([lambda: Monitor(mk(0), os.path.join("models/ppo_vec", "log_file"))])
    driver = reference_sb_helper.SBPolicy(env, DummyVecEnv([lambda: mk(1)]), config, "models/ppo_vec", algo="PPO")
    with pytest.raises(AttributeError, match="save"):
        driver.learn()
    assert os.path.isfile("models/ppo_vec/ppo_vec.zip")
    rows = open("tensorboard_logs/models/ppo_vec/PPO2_1/scalars.csv").read()
    assert "success_rate" in rows and "loss/value_function_loss" in rows
    model = sb.PPO2.load("models/ppo_vec/ppo_vec.zip")
    assert model.get_vec_normalize_env() is None and model.get_parameters()["model/pi/w:0"].shape == (64, 3)
