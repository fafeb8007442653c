"""The reference's own ``SBPolicy(..., algo="TRPO").learn()`` and ``.save()`` (manipulation_main/training/sb_helper.py:129-136:
``sb.TRPO(MlpPolicy, env, verbose=2, gamma=..., timesteps_per_batch=config['TRPO']['max_iters'],
vf_stepsize=config['TRPO']['step_size'], tensorboard_log=...)``) on the ``TRPO`` section config/simplified_object_picking.yaml
ships (max_iters 400, step_size 0.01; total_timesteps cut to two batches), then the loader of ``run`` (train_stable_baselines.py:
95-96 ``sb.TRPO.load``): imported from where it lies, unmodified, on top of the alias package, the emulation build and
tests/fake_env.py -- the set-up of tests/test_reference_driver_ppo.py.  Skipped where /root/reference does not exist (the GPU box)."""
import importlib
import os
import sys
import types

import numpy as np
import pytest

import stable_baselines as sb
from fake_env import FakeGraspEnv
from grasp_rl.engine import TrpoEngine
from grasp_rl.sb import spaces
from grasp_rl.sb.trpo import TRPO
from hostemu_backend import NumpyHostBackend
from stable_baselines.bench import Monitor
from stable_baselines.common.vec_env import DummyVecEnv

REF_TRAINING = "/root/reference/manipulation_main/training"
REF_CONFIG = "/root/reference/config/simplified_object_picking.yaml"
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
    monkeypatch.delenv("GRL_DATA_PARALLEL", raising=False)
    for name in ("sb_helper", "base_callbacks", "custom_obs_policy"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    monkeypatch.setattr(TRPO, "_engine_factory", staticmethod(
        lambda cfg, trpo, device: TrpoEngine(cfg, trpo, backend=NumpyHostBackend(), lib_path=hostemu_lib)))
    mod = importlib.import_module("sb_helper")
    assert os.path.realpath(mod.__file__).startswith("/root/reference/")
    yield mod
    for name in ("sb_helper", "base_callbacks", "custom_obs_policy"):
        sys.modules.pop(name, None)


def _scalar(v):
    for cast in (int, float):
        try:
            return cast(v)
        except ValueError:
            pass
    return None if v in ("", "null", "~") else v


def _shipped_trpo_section():
    """The `TRPO:` block of the shipped yaml, read without a yaml package: the `key: value` lines indented under it."""
    out, inside = {}, False
    for line in open(REF_CONFIG):
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        if not line.startswith((" ", "\t")):
            inside = line.split(":")[0].strip() == "TRPO"
        elif inside:
            k, v = line.split("#")[0].split(":", 1)
            out[k.strip()] = _scalar(v.strip())
    return out


def test_reference_sbpolicy_trpo_learn_save_and_the_loader_of_run(reference_sb_helper, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("models/trpo_vec")
    section = _shipped_trpo_section()
    assert section["max_iters"] == 400 and section["step_size"] == 0.01 and section["total_timesteps"] == 1000000
    section["total_timesteps"] = 800      # two batches
    assert section["tensorboard_logs"] == "tensorboard_logs/trpo_1m"      # tensorboard on: TensorboardCallback writes through locals['writer']
    config = {"normalize": False, "discount_factor": 0.99, "TRPO": section}
    mk = lambda s: FakeGraspEnv(vector_dim=101, seed=s)
    env = DummyVecEnv([lambda: Monitor(mk(0), os.path.join("models/trpo_vec", "log_file"))])
    driver = reference_sb_helper.SBPolicy(env, DummyVecEnv([lambda: mk(1)]), config, "models/trpo_vec", None, "TRPO")
    driver.learn()                                            # ends in SBPolicy.save
    assert os.path.isfile("models/trpo_vec/trpo_vec.zip")
    rows = open("tensorboard_logs/models/trpo_vec/TRPO_1/scalars.csv").read()
    assert "loss/approximate_kullback-leibler" in rows
    model = sb.TRPO.load("models/trpo_vec/trpo_vec.zip")      # train_stable_baselines.py:95-96
    assert model.timesteps_per_batch == 400 and model.vf_stepsize == 0.01 and model.gamma == 0.99 and model.max_kl == 0.01
    P = model.get_parameters()
    assert P["model/pi_fc0/w:0"].shape == (101, 64) and P["model/pi/logstd:0"].shape == (1, 5)
    assert all(np.isfinite(v).all() for v in P.values())
    a, _ = model.predict(mk(2).reset(), deterministic=True)
    assert a.shape == (5,) and (np.abs(a) <= 1).all()
