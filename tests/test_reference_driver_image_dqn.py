"""The reference's own ``SBPolicy(..., algo="DQN").learn()`` (manipulation_main/training/sb_helper.py:155-177: ``sb.DQN(
DQNMlpPolicy, env, ...)``) on the IMAGE environment, as ``train_stable_baselines.py train --config config/gripper_grasp.yaml
--algo DQN`` reaches it (depth_observation: True, discrete actuator): imported from where it lies, unmodified, on top of the alias
package, the emulation build and tests/fake_env.py -- the set-up of tests/test_reference_driver.py.  Skipped where /root/reference
does not exist (the GPU box)."""
import importlib
import os
import sys
import types

import numpy as np
import pytest

import stable_baselines as sb
from fake_env import FakeGraspEnv
from grasp_rl.engine import QEngine
from grasp_rl.sb import spaces
from grasp_rl.sb.dqn import DQN
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
    for name in ("sb_helper", "base_callbacks", "custom_obs_policy"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    monkeypatch.setattr(DQN, "_engine_factory",
                        staticmethod(lambda cfg, device: QEngine(cfg, backend=NumpyHostBackend(), lib_path=hostemu_lib)))
    mod = importlib.import_module("sb_helper")
    assert os.path.realpath(mod.__file__).startswith("/root/reference/")
    yield mod
    for name in ("sb_helper", "base_callbacks", "custom_obs_policy"):
        sys.modules.pop(name, None)


def test_reference_sbpolicy_dqn_on_the_image_env(reference_sb_helper, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("models/dqn_img")
    config = {"normalize": False, "discount_factor": 0.99,
              "DQN": {"tensorboard_logs": None, "batch_size": 8, "prioritized_replay": False, "total_timesteps": 1030}}
    mk = lambda s: FakeGraspEnv("depth", seed=s, discrete_actions=6)
    env = DummyVecEnv([lambda: Monitor(mk(0), os.path.join("models/dqn_img", "log_file"))])
    driver = reference_sb_helper.SBPolicy(env, DummyVecEnv([lambda: mk(1)]), config, "models/dqn_img", algo="DQN")
    driver.learn()                                            # (learning_starts is stable-baselines' 1000: thirty updates)
    assert os.path.isfile("models/dqn_img/dqn_img.zip")
    model = sb.DQN.load("models/dqn_img/dqn_img.zip")
    assert tuple(model.observation_space.shape) == (64, 64, 2)
    P = model.get_parameters()
    assert P["deepq/model/action_value/fully_connected/weights:0"].shape == (8192, 64)
    assert all(np.isfinite(v).all() for v in P.values())
    obs = mk(2).reset()
    a, _ = model.predict(obs, deterministic=True)
    assert 0 <= int(a) < 6
    a, _ = model.predict(obs[None], deterministic=True)
    assert a.shape == (1,) and 0 <= int(a[0]) < 6
