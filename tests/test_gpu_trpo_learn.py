"""``TRPO`` end to end on the MI355X: the learn loop of grasp_rl/sb/trpo.py over a real handle -- vector observations (one-launch
act) and the 64 x 64 x 2 image of gripper_grasp.yaml flattened to 8192 values (launch list, first layer in partial sums) -- then
save / load / predict, and a policy that learns the one-step task of tests/test_gpu_ppo2_learn.py."""
import numpy as np
import pytest

import stable_baselines as sb
from fake_env import FakeGraspEnv
from stable_baselines.common.policies import MlpPolicy
from stable_baselines.common.vec_env import DummyVecEnv
from test_gpu_ppo2_learn import _Target

pytestmark = pytest.mark.gpu


def _updates(model, total):
    """learn() batch by batch so that the metrics of EVERY update can be read."""
    out, T = [], model.timesteps_per_batch
    for _ in range(total // T):
        model.learn(total_timesteps=T, reset_num_timesteps=False)
        out.append(model.engine.metrics())
    return out


def test_learn_save_load_predict_on_vector_observations(tmp_path):
    env = DummyVecEnv([lambda: FakeGraspEnv(vector_dim=101, seed=0, episode_len=5)])
    model = sb.TRPO(MlpPolicy, env, timesteps_per_batch=130, seed=1)
    p0 = model.get_parameters()
    model.learn(total_timesteps=260)
    assert model.num_timesteps == 260
    p1 = model.get_parameters()
    for n in p0:
        assert np.isfinite(p1[n]).all() and np.array_equal(p0[n], p1[n]) == n.startswith("model/q/"), n
    m = model.engine.metrics()
    assert m["ls_index"] >= 0 and m["trial_meankl"] <= 1.5 * 0.01 and m["cg_iters"] == 10
    path = model.save(str(tmp_path / "trpo"))
    loaded = sb.TRPO.load(path)
    obs = env.reset()
    a, _ = model.predict(obs, deterministic=True)
    b, _ = loaded.predict(obs, deterministic=True)
    assert a.shape == (1, 5) and np.array_equal(a, b) and (np.abs(a) <= 1).all()


def test_learn_save_load_predict_on_the_flattened_image(tmp_path):
    env = DummyVecEnv([lambda: FakeGraspEnv("depth", seed=0)])
    model = sb.TRPO(MlpPolicy, env, timesteps_per_batch=130, seed=0)
    p0 = model.get_parameters()
    assert p0["model/pi_fc0/w:0"].shape == (8192, 64)
    model.learn(total_timesteps=130)
    p1 = model.get_parameters()
    assert all(np.isfinite(v).all() for v in p1.values())
    assert not np.array_equal(p0["model/vf_fc0/w:0"], p1["model/vf_fc0/w:0"])
    m = model.engine.metrics()
    assert m["ls_index"] < 0 or not np.array_equal(p0["model/pi_fc0/w:0"], p1["model/pi_fc0/w:0"])
    loaded = sb.TRPO.load(model.save(str(tmp_path / "trpo_img")))
    obs = env.reset()[0]
    a, _ = model.predict(obs, deterministic=True)
    b, _ = loaded.predict(obs, deterministic=True)
    assert a.shape == (5,) and np.array_equal(a, b) and (np.abs(a) <= 1).all()


def test_the_policy_improves_on_a_one_step_task():
    """One-step episodes, gamma 0, one environment, timesteps_per_batch 128, every other argument at its default.

    The step count comes from the float64 restatement of tests/trpo_util.py (`one_step_task_table`: `Ref.update` driven by a host
    loop over the same task, eight seeds; after / before of the mean squared distance of the mean action from its target after n
    batches of 128 steps; `python tests/trpo_util.py` prints it):

        seed      10     20     30     40     50     60
        0      0.475  0.288  0.294  0.195  0.154  0.151
        1      0.330  0.357  0.257  0.160  0.058  0.072
        2      0.224  0.428  0.454  0.244  0.103  0.064
        3      0.365  0.349  0.290  0.172  0.051  0.061
        4      0.415  0.492  0.307  0.174  0.079  0.051
        5      0.429  0.689  0.400  0.430  0.212  0.181
        6      0.455  0.377  0.337  0.278  0.254  0.075
        7      0.422  0.545  0.379  0.257  0.094  0.078
        worst  0.475  0.689  0.454  0.430  0.254  0.181

    50 batches (128 x 50 steps) is the smallest multiple of 128 x 10 at which the worst seed is at or below 0.35; the assertion is
    after < 0.5 before.  Every accepted update must have kept meankl <= 1.5 max_kl."""
    env = DummyVecEnv([lambda: _Target(0)])
    model = sb.TRPO(MlpPolicy, env, timesteps_per_batch=128, gamma=0.0, seed=0)
    probe = np.random.default_rng(9).uniform(-1, 1, (64, 4)).astype(np.float32)
    target = 0.5 * np.sign(probe[:, :1])

    def err():
        return float(np.mean((model.predict(probe, deterministic=True)[0] - target) ** 2))
    before = err()
    ms = _updates(model, 128 * 50)
    after = err()
    accepted = [m for m in ms if m["ls_index"] >= 0]
    print("mean squared distance of the mean action from its target: %.4f -> %.4f; %d of %d updates accepted, largest meankl %.5f"
          % (before, after, len(accepted), len(ms), max(m["trial_meankl"] for m in accepted)))
    assert model.num_timesteps == 128 * 50 and len(accepted) > 0
    assert all(m["trial_meankl"] <= 1.5 * model.max_kl for m in accepted)
    assert after < 0.5 * before
