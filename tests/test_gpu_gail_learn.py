"""``GAIL`` end to end on the MI355X: the learn loop of grasp_rl/sb/gail.py over a real handle -- rollouts whose rewards the
discriminator writes on the device, TRPO steps on them, discriminator updates from the last rollout and the expert table -- on a
one-step task whose environment pays nothing: all the policy can learn from is the expert's demonstrations."""
import numpy as np
import pytest

import stable_baselines as sb
from grasp_rl.sb.spaces import Box
from stable_baselines.common.policies import MlpPolicy
from stable_baselines.common.vec_env import DummyVecEnv
from stable_baselines.gail import ExpertDataset, generate_expert_traj

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2, 3, 4)
# Measured on one MI355X over SEEDS with LEARN below, before -> after: 0.2474 -> 0.0806, 0.2507 -> 0.0656,
# 0.2505 -> 0.0769, 0.2504 -> 0.0677, 0.2502 -> 0.0711; the worst ratio is 0.326 and the bound lies halfway between it and 1.
RATIO = 0.663
LEARN = dict(timesteps_per_batch=128, g_step=1, d_step=8, d_stepsize=3e-3, hidden_size_adversary=32, gamma=0.0, vf_iters=3, iterations=40)


class _Silent:
    """One-step episodes like _Target of tests/test_gpu_ppo2_learn.py, but the environment always returns reward 0."""
    observation_space = Box(-1.0, 1.0, shape=(4,), dtype=np.float32)
    action_space = Box(-1.0, 1.0, shape=(1,), dtype=np.float32)

    def __init__(self, seed):
        self._rng = np.random.default_rng(seed)

    def reset(self):
        self._o = self._rng.uniform(-1, 1, 4).astype(np.float32)
        return self._o

    def step(self, action):
        return self.reset(), 0.0, True, {}

    def close(self):
        pass


def expert(obs):
    return np.array([0.5 * np.sign(obs[0])], np.float32)


def run(seed, model_factory=None):
    """(mean squared distance of the deterministic action from the expert's on 64 probe observations) before and after learn"""
    np.random.seed(seed)
    data = generate_expert_traj(expert, None, _Silent(100 + seed), n_episodes=512)
    dataset = ExpertDataset(traj_data=data, verbose=0)
    kw = dict(LEARN)
    iterations = kw.pop("iterations")
    model = (model_factory or sb.GAIL)(MlpPolicy, DummyVecEnv([lambda: _Silent(seed)]), dataset, seed=seed, **kw)
    probe = np.random.default_rng(9).uniform(-1, 1, (64, 4)).astype(np.float32)
    target = 0.5 * np.sign(probe[:, :1])

    def err():
        acts = np.concatenate([model.predict(probe[k:k + 1], deterministic=True)[0] for k in range(64)])
        return float(np.mean((acts - target) ** 2))
    before = err()
    model.learn(total_timesteps=kw["timesteps_per_batch"] * iterations)
    after = err()
    assert model.num_timesteps == kw["timesteps_per_batch"] * iterations
    assert min(model.rew_buffer) > 0 and not any(model.true_rew_buffer)      # discriminator returns; the environment paid nothing
    return before, after


def test_the_policy_moves_towards_the_expert_on_a_task_that_pays_nothing():
    before, after = run(0)
    print("mean squared distance of the mean action from the expert's: %.4f -> %.4f" % (before, after))
    assert np.isfinite(after) and after < RATIO * before
