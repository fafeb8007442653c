"""sb.SAC(CnnPolicy) on a camera that is not 64x64: the reference builds its observation space from config/camera_info.yaml
(sensor.py:36-41), so an 84x84 camera is a configuration change there.  Construction, learn, predict, the parameter table,
save / load and the refusals, on the TEST-ONLY g++ emulation build."""
import numpy as np
import pytest

import sac_image_size_util as su
import stable_baselines as sb
from fake_env import FakeGraspEnv
from grasp_rl._capi import GrlError
from grasp_rl.engine import SacEngine
from grasp_rl.sb.sac import SAC
from grasp_rl.sb.spaces import Box
from hostemu_backend import NumpyHostBackend
from stable_baselines.common.vec_env import DummyVecEnv, VecNormalize
from stable_baselines.sac.policies import CnnPolicy as sacCnn
from test_sb_api_host import create_augmented_nature_cnn

KW = {"layers": [64, 64], "cnn_extractor": create_augmented_nature_cnn(1)}


@pytest.fixture
def emulated_engine(hostemu_lib, monkeypatch):
    monkeypatch.setattr(SAC, "_engine_factory",
                        staticmethod(lambda cfg, device: SacEngine(cfg, backend=NumpyHostBackend(), lib_path=hostemu_lib)))


def _env(hw, seed=0):
    return VecNormalize(DummyVecEnv([lambda: su.SizedGraspEnv(hw, "depth", seed=seed)]), norm_obs=True, norm_reward=True, clip_obs=10.)


def test_sac_on_an_84x84_camera(tmp_path, emulated_engine):
    env = _env(84)
    assert env.observation_space.shape == (84, 84, 2)
    model = sb.SAC(sacCnn, env, policy_kwargs=KW, buffer_size=64, batch_size=4, learning_starts=8, seed=3)
    cfg = model.engine.cfg
    assert (cfg.img_hw, cfg.extractor, cfg.obs_channels, cfg.n_direct, cfg.normalize) == (84, 1, 2, 1, 1)
    P0 = model.get_parameters()
    for scope in ("model/pi", "model/values_fn", "target/values_fn"):
        assert P0[scope + "/cnn_fc1/w:0"].shape == (3136, 512)
    assert np.array_equal(P0["target/values_fn/cnn_fc1/w:0"], P0["model/values_fn/cnn_fc1/w:0"])
    assert abs(float(np.std(P0["model/pi/cnn_fc1/w:0"]))) > 0                       # initialised over the engine's table
    model.learn(40)
    assert model.num_timesteps == 40 and model.n_updates == 40 - 8 + 1
    P1 = model.get_parameters()
    assert all(np.isfinite(v).all() for v in P1.values())
    assert not np.array_equal(P0["model/pi/cnn_fc1/w:0"], P1["model/pi/cnn_fc1/w:0"])
    env.training = False
    obs = env.reset()
    one, _ = model.predict(obs[0], deterministic=True)
    many, _ = model.predict(np.concatenate([obs] * 3), deterministic=True)
    assert one.shape == (5,) and many.shape == (3, 5) and np.all(np.abs(many) <= 1) and np.allclose(many, one[None], atol=1e-6)
    # save / load: the observation space, the parameters and the predictions come back
    path = str(tmp_path / "sac84")
    model.save(path)
    again = sb.SAC.load(path)
    assert again.observation_space.shape == (84, 84, 2) and again.engine.cfg.img_hw == 84
    P2 = again.get_parameters()
    assert list(P2) == list(P1) and all(np.array_equal(P1[n], P2[n]) for n in P1)
    assert np.array_equal(again.predict(obs, deterministic=True)[0], model.predict(obs, deterministic=True)[0])
    # the weights of a 64x64 model do not fit: refused with both shapes named
    small = sb.SAC(sacCnn, DummyVecEnv([lambda: FakeGraspEnv("depth", seed=1)]), policy_kwargs=KW, buffer_size=16, batch_size=4)
    small.save(str(tmp_path / "sac64"))
    with pytest.raises(GrlError, match=r"model/pi/cnn_fc1/w:0: expected shape \(3136, 512\) \(1605632 values\), got shape \(1024, 512\)"):
        model.load_parameters(sb.SAC.load(str(tmp_path / "sac64")).get_parameters())
    assert all(np.array_equal(P1[n], v) for n, v in model.get_parameters().items() if "cnn_fc1" in n)


class _BoxEnv(FakeGraspEnv):
    def __init__(self, shape):
        super().__init__("depth")
        self.observation_space = Box(0, 255, shape=shape, dtype=np.float32)


@pytest.mark.parametrize("shape, words", [((64, 84, 2), "height 64 and width 84 differ"), ((84, 64, 2), "height 84 and width 64 differ"),
                                          ((32, 32, 2), "36x36 to 128x128, got 32x32"), ((132, 132, 2), "36x36 to 128x128, got 132x132"),
                                          ((35, 35, 2), "36x36 to 128x128, got 35x35"), ((129, 129, 2), "36x36 to 128x128, got 129x129")])
def test_rectangular_and_out_of_range_images_are_refused_in_words(emulated_engine, shape, words):
    with pytest.raises(ValueError, match=words):
        sb.SAC(sacCnn, DummyVecEnv([lambda: _BoxEnv(shape)]), policy_kwargs=KW, buffer_size=16, batch_size=4)


@pytest.mark.parametrize("hw", [36, 128])
def test_the_ends_of_the_range_construct(emulated_engine, hw):
    model = sb.SAC(sacCnn, DummyVecEnv([lambda: su.SizedGraspEnv(hw, "depth")]), policy_kwargs=KW, buffer_size=8, batch_size=2)
    assert model.get_parameters()["model/pi/cnn_fc1/w:0"].shape == (su.dense_k(hw), 512)
    a, _ = model.predict(model.env.reset(), deterministic=True)
    assert a.shape == (1, 5) and np.isfinite(a).all()
