"""The reference's OWN command line on a camera of 84x84:
    GRL_NUM_ENVS=16 ... train_stable_baselines.py train --config <yaml> --algo SAC
with `sensor.camera_info` of the configuration pointing at a camera_info.yaml of height 84 / width 84 (the reference builds the
observation space from it, sensor.py:36-41).  `train(args)` is imported from where the reference lies, unmodified; the simulator
is the fake one, which reads the camera file the way the reference's sensor does; the engine is the TEST-ONLY emulation build.
Skipped where /root/reference does not exist (the GPU box)."""
import enum
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

import sac_image_size_util as su
import stable_baselines as sb
from grasp_rl.sb.sac import SAC
from test_reference_driver import REF_TRAINING, reference_sb_helper  # noqa: F401  (the fixture)

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF_TRAINING, "sb_helper.py")),
                                reason="/root/reference is not present on this box")


def test_reference_train_script_on_an_84x84_camera_with_16_envs(reference_sb_helper, tmp_path, monkeypatch):  # noqa: F811
    import yaml

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    robot = types.ModuleType("manipulation_main.gripperEnv.robot")
    robot.RobotEnv = type("RobotEnv", (), {"Status": enum.IntEnum("Status", {"RUNNING": 0, "SUCCESS": 1})})
    wrapper = types.ModuleType("manipulation_main.training.wrapper")
    wrapper.TimeFeatureWrapper = lambda env: env
    pkgs = {n: types.ModuleType(n) for n in ("manipulation_main", "manipulation_main.gripperEnv", "manipulation_main.training",
                                             "manipulation_main.common")}
    for m in pkgs.values():
        m.__path__ = []
    pkgs.update({"manipulation_main.gripperEnv.robot": robot, "manipulation_main.training.wrapper": wrapper})
    for n, m in pkgs.items():
        monkeypatch.setitem(sys.modules, n, m)
    real_yaml_load = yaml.load
    monkeypatch.setattr(yaml, "load", lambda f, Loader=None: real_yaml_load(f, Loader=Loader or yaml.FullLoader))
    io_utils = load("manipulation_main.common.io_utils", "/root/reference/manipulation_main/common/io_utils.py")
    monkeypatch.setitem(sys.modules, "manipulation_main.common.io_utils", io_utils)
    pkgs["manipulation_main.common"].io_utils = io_utils
    utils = load("manipulation_main.utils", "/root/reference/manipulation_main/utils.py")
    monkeypatch.setitem(sys.modules, "manipulation_main.utils", utils)
    made = []

    def make(name, config=None, **kw):
        assert name == "gripper-env-v0"
        with open(config["sensor"]["camera_info"]) as f:            # what the reference's sensor reads: height / width
            cam = yaml.safe_load(f)
        assert cam["height"] == cam["width"]
        made.append(os.getpid())
        return su.SizedGraspEnv(cam["height"], "depth", seed=len(made) + 17 * (os.getpid() % 1000), episode_len=5)
    sys.modules["gym"].make = make
    monkeypatch.delitem(sys.modules, "train_stable_baselines", raising=False)
    script = importlib.import_module("train_stable_baselines")
    assert os.path.realpath(script.__file__).startswith("/root/reference/")
    with open("/root/reference/config/gripper_grasp.yaml") as f:
        cfg = yaml.safe_load(f)
    assert cfg["sensor"]["camera_info"] == "config/camera_info.yaml"
    monkeypatch.chdir(tmp_path)
    with open("camera_info_84.yaml", "w") as f:
        yaml.safe_dump({"height": 84, "width": 84, "near": 0.02, "far": 2.0}, f)
    cfg["sensor"]["camera_info"] = str(tmp_path / "camera_info_84.yaml")
    cfg["SAC"]["buffer_size"], cfg["SAC"]["batch_size"] = 256, 4
    os.makedirs("trained")
    with open("cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setenv("GRL_NUM_ENVS", "16")
    monkeypatch.setenv("GRL_ENV_START_METHOD", "fork")
    seen = {}
    real_learn = SAC.learn

    def spy(self, total_timesteps, callback=None, **kw):
        seen["n_envs"], seen["act_batch"], seen["img_hw"] = self.n_envs, self.engine.cfg.act_batch, self.engine.cfg.img_hw
        seen["space"] = tuple(self.observation_space.shape)
        out = real_learn(self, total_timesteps, callback=callback, **kw)
        seen["updates"], seen["steps"] = self.n_updates, self.num_timesteps
        return out
    monkeypatch.setattr(SAC, "learn", spy)
    args = types.SimpleNamespace(config="cfg.yaml", model_dir="trained/cam84", algo="SAC", load_dir=None, timestep="112",
                                 simple=False, shaped=False, visualize=False, timefeature=False)
    script.train(args)
    assert seen["n_envs"] == seen["act_batch"] == 16 and seen["img_hw"] == 84 and seen["space"] == (84, 84, 2)
    # one update per environment step once learning_starts (100) is reached: of the vectorised steps 16, 32, .. 112 only the last
    assert seen["steps"] == 112 and seen["updates"] == 16
    assert os.path.isfile("trained/cam84/cam84.zip") and os.path.isfile("trained/cam84/vecnormalize.pkl")
    model = sb.SAC.load("trained/cam84/cam84.zip")
    P = model.get_parameters()
    assert P["model/pi/cnn_fc1/w:0"].shape == (3136, 512) and all(np.isfinite(v).all() for v in P.values())
    assert made.count(os.getpid()) == 2                                        # template train env + evaluation env; 16 in workers
    sys.modules.pop("train_stable_baselines", None)
