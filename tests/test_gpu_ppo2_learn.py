"""``PPO2`` end to end on the MI355X: the learn loop of grasp_rl/sb/ppo2.py over a real handle -- vector observations (one-launch
act) with three environments, and the 64 x 64 x 2 image of gripper_grasp.yaml flattened to 8192 values (launch list, first layer
in partial sums) -- then save / load / predict, and a policy that learns a one-step task."""
import numpy as np
import pytest

import stable_baselines as sb
from fake_env import FakeGraspEnv
from grasp_rl.sb.spaces import Box
from stable_baselines.common.policies import MlpPolicy
from stable_baselines.common.vec_env import DummyVecEnv

pytestmark = pytest.mark.gpu


def test_learn_save_load_predict_on_vector_observations(tmp_path):
    env = DummyVecEnv([(lambda k=k: FakeGraspEnv(vector_dim=101, seed=k, episode_len=5)) for k in range(3)])
    model = sb.PPO2(MlpPolicy, env, n_steps=8, nminibatches=4, noptepochs=2, seed=1)
    p0 = model.get_parameters()
    model.learn(total_timesteps=48)
    assert model.num_timesteps == 48 and model.n_updates == 2 * 4 * 2
    p1 = model.get_parameters()
    for n in p0:
        assert np.isfinite(p1[n]).all() and np.array_equal(p0[n], p1[n]) == n.startswith("model/q/"), n
    path = model.save(str(tmp_path / "ppo"))
    loaded = sb.PPO2.load(path)
    obs = env.reset()
    a, _ = model.predict(obs, deterministic=True)
    b, _ = loaded.predict(obs, deterministic=True)
    assert a.shape == (3, 5) and np.array_equal(a, b) and (np.abs(a) <= 1).all()


def test_learn_on_the_flattened_image():
    env = DummyVecEnv([lambda: FakeGraspEnv("depth", seed=0)])
    model = sb.PPO2(MlpPolicy, env, n_steps=16, nminibatches=2, noptepochs=2, seed=0)
    p0 = model.get_parameters()
    assert p0["model/pi_fc0/w:0"].shape == (8192, 64)
    model.learn(total_timesteps=32)
    p1 = model.get_parameters()
    assert all(np.isfinite(v).all() for v in p1.values())
    assert not np.array_equal(p0["model/vf_fc0/w:0"], p1["model/vf_fc0/w:0"]) and not np.array_equal(p0["model/pi/logstd:0"], p1["model/pi/logstd:0"])
    a, _ = model.predict(env.reset()[0], deterministic=True)
    assert a.shape == (5,) and (np.abs(a) <= 1).all()


class _Target:
    """One-step episodes: reward = -|a - 0.5 sign(obs_0)|^2 -- the mean has to follow the observation."""
    observation_space = Box(-1.0, 1.0, shape=(4,), dtype=np.float32)
    action_space = Box(-1.0, 1.0, shape=(1,), dtype=np.float32)

    def __init__(self, seed):
        self._rng = np.random.default_rng(seed)

    def reset(self):
        self._o = self._rng.uniform(-1, 1, 4).astype(np.float32)
        return self._o

    def step(self, action):
        r = -float((float(action[0]) - 0.5 * np.sign(self._o[0])) ** 2)
        return self.reset(), r, True, {}

    def close(self):
        pass


def test_the_policy_improves_on_a_one_step_task():
    env = DummyVecEnv([(lambda k=k: _Target(k)) for k in range(4)])
    model = sb.PPO2(MlpPolicy, env, n_steps=32, nminibatches=4, noptepochs=4, seed=0, learning_rate=3e-3, gamma=0.0, ent_coef=0.0)
    probe = np.random.default_rng(9).uniform(-1, 1, (64, 4)).astype(np.float32)
    target = 0.5 * np.sign(probe[:, :1])

    def err():
        acts = np.concatenate([model.predict(probe[k:k + 4], deterministic=True)[0] for k in range(0, 64, 4)])
        return float(np.mean((acts - target) ** 2))
    before = err()
    model.learn(total_timesteps=128 * 30)
    after = err()
    print("mean squared distance of the mean action from its target: %.4f -> %.4f" % (before, after))
    assert after < 0.5 * before
