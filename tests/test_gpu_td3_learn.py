"""Evidence that the TD3 update path LEARNS, as tests/test_gpu_learning.py shows it for SAC / DQN / BDQ: ReachGraspEnv on the 101-d
vector observations with Box actions through VecNormalize -> TD3.learn -> the reference's deterministic evaluation
(grasp_rl.synthetic.learn_reach("td3", "vector")).  A uniformly random policy succeeds in 0.07 of the episodes."""
import numpy as np
import pytest

from grasp_rl import synthetic

pytestmark = pytest.mark.gpu

STEPS = 32_000


def test_td3_learns_to_reach_through_model_learn():
    """TD3 + MlpPolicy [64, 64], 16 envs, batch 256, lr 3e-4, policy_delay 2, NormalActionNoise(0, 0.1) per environment, one
    update per environment step, 32 000 steps (31 760 updates; 3.4 s of learn on the MI355X).  Measured on the MI355X, seeds
    0 / 1 / 2: training success (last 200 episodes) 0.475 / 0.72 / 0.555, deterministic evaluation over 200 episodes
    0.67 / 0.875 / 0.645, mean final distance 0.261 / 0.180 / 0.262.  The lowest evaluation, 0.645, is nine times the random
    policy's 0.07.  Asserted for seed 0 at 0.1 -- three standard deviations of a 200-episode estimate -- below that lowest."""
    r = synthetic.learn_reach("td3", "vector", total_timesteps=STEPS, n_envs=16, seed=0)
    print(r)
    assert np.isfinite(r["metrics"]).all()
    assert r["updates"] >= STEPS - 16 * 17 and r["targets_moved"] == r["targets"] == 18
    assert r["eval_success"] >= 0.545 and r["eval_distance"] <= 0.36, r
