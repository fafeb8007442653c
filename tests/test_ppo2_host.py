"""``PPO2`` -- the stable-baselines surface the reference drives with ``--algo PPO`` (sb_helper.py:137-154, loader
train_stable_baselines.py:99-100) -- on the emulation build: the learn loop's counters and callback protocol, seeded
reproducibility, N environments, learning-rate schedules, save / load, predict, and everything the class refuses by name."""
import os

import numpy as np
import pytest

import stable_baselines as sb
from fake_env import FakeGraspEnv
from grasp_rl.engine import PpoEngine
from grasp_rl.sb import spaces
from grasp_rl.sb.callbacks import BaseCallback
from grasp_rl.sb.ppo2 import PPO2
from hostemu_backend import NumpyHostBackend
from stable_baselines.bench import Monitor
from stable_baselines.common.policies import CnnPolicy, MlpPolicy
from stable_baselines.common.vec_env import DummyVecEnv


@pytest.fixture
def emulated(monkeypatch, hostemu_lib):
    monkeypatch.delenv("GRL_NUM_ENVS", raising=False)
    monkeypatch.setattr(PPO2, "_engine_factory", staticmethod(
        lambda cfg, ppo, device: PpoEngine(cfg, ppo, backend=NumpyHostBackend(), lib_path=hostemu_lib)))


class Recorder(BaseCallback):
    def __init__(self, stop_at=None):
        super().__init__()
        self.steps, self.starts, self.ends, self.stop_at, self.writers, self.timesteps = 0, 0, 0, stop_at, [], []

    def _on_rollout_start(self):
        self.starts += 1

    def _on_rollout_end(self):
        self.ends += 1

    def _on_step(self):
        self.steps += 1
        self.writers.append(self.locals.get("writer"))
        self.timesteps.append(self.num_timesteps)
        assert self.locals["clipped_actions"].min() >= -1.0 and self.locals["clipped_actions"].max() <= 1.0
        return self.stop_at is None or self.steps < self.stop_at


def _env(n=1, dim=11, tmp=None):
    def mk(k):
        e = FakeGraspEnv(vector_dim=dim, seed=k, episode_len=5)
        return (lambda: Monitor(e, os.path.join(str(tmp), "log_%d" % k))) if tmp is not None else (lambda: e)
    return DummyVecEnv([mk(k) for k in range(n)])


def test_the_alias_is_the_real_class(emulated):
    assert sb.PPO2 is PPO2
    from grasp_rl import sb as gsb
    assert gsb.PPO2 is PPO2


def test_learn_counts_and_moves_every_trainable_tensor(emulated, tmp_path):
    model = sb.PPO2(MlpPolicy, _env(tmp=tmp_path), n_steps=8, nminibatches=2, noptepochs=3, seed=3, gamma=0.97, learning_rate=1e-3)
    assert [n for n in model.get_parameters()][:4] == ["model/pi_fc0/w:0", "model/pi_fc0/b:0", "model/vf_fc0/w:0", "model/vf_fc0/b:0"]
    p0 = model.get_parameters()
    assert not p0["model/pi/logstd:0"].any() and not p0["model/pi/b:0"].any() and p0["model/pi_fc0/w:0"].shape == (11, 64)
    assert np.allclose(p0["model/pi_fc0/w:0"] @ p0["model/pi_fc0/w:0"].T, 2.0 * np.eye(11), atol=1e-5)      # orthogonal rows, gain sqrt 2
    assert np.allclose(p0["model/vf/w:0"].T @ p0["model/vf/w:0"], 1.0, atol=1e-5)
    assert np.abs(p0["model/pi/w:0"]).max() <= 0.01
    rec = Recorder()
    model.learn(total_timesteps="43", callback=rec)           # (the reference's --timestep arrives as a string) 43 // 8 = 5 rollouts
    assert rec.steps == 40 and model.num_timesteps == 40 and rec.starts == 5 and rec.ends == 5
    assert rec.timesteps[:3] == [1, 2, 3] and model.n_updates == 5 * 2 * 3
    p1 = model.get_parameters()
    for n in p0:
        assert np.array_equal(p0[n], p1[n]) == n.startswith("model/q/"), n
    assert all(np.isfinite(v).all() for v in p1.values())
    assert len(model.ep_info_buf) == 8 and model.ep_info_buf[0]["l"] == 5      # Monitor episodes of five steps
    assert model.get_env().num_envs == 1 and model.get_vec_normalize_env() is None


def test_same_seed_same_parameters_and_a_stop_from_on_step(emulated):
    P = []
    for _ in range(2):
        model = sb.PPO2(MlpPolicy, _env(), n_steps=6, nminibatches=3, noptepochs=2, seed=11)
        model.learn(total_timesteps=12)
        P.append(model.get_parameters())
    assert all(np.array_equal(P[0][n], P[1][n]) for n in P[0])
    model = sb.PPO2(MlpPolicy, _env(), n_steps=6, nminibatches=3, noptepochs=2, seed=11)
    rec = Recorder(stop_at=9)
    model.learn(total_timesteps=600, callback=rec)
    assert rec.steps == 9 and model.num_timesteps == 9 and model.n_updates == 6       # one rollout trained, the second abandoned
    model.learn(total_timesteps=6)                             # the slot the stop left open does not block the next run
    assert model.num_timesteps == 6


def test_n_environments_and_schedule_and_writer(emulated, tmp_path, monkeypatch):
    seen = []
    lr = lambda frac: seen.append(frac) or 1e-3 * frac
    model = sb.PPO2(MlpPolicy, _env(n=3), n_steps=4, nminibatches=4, noptepochs=1, seed=0, learning_rate=lr,
                    tensorboard_log=str(tmp_path / "tb"), verbose=1)
    assert model.n_batch == 12 and model.engine.cfg.batch_size == 3 and model.engine.cfg.act_batch == 3
    seen.clear()
    rec = Recorder()
    model.learn(total_timesteps=36, callback=rec, tb_log_name="PPO2")
    assert rec.steps == 12 and model.num_timesteps == 36 and rec.timesteps[:2] == [3, 6]
    assert seen == [1.0, 1.0 - 1.0 / 3.0, 1.0 - 2.0 / 3.0]     # evaluated once per rollout
    assert all(w is not None and hasattr(w, "add_summary") for w in rec.writers)
    rows = open(os.path.join(str(tmp_path / "tb"), "PPO2_1", "scalars.csv")).read()
    assert "loss/policy_gradient_loss" in rows and "input_info/learning_rate" in rows
    with pytest.raises(ValueError, match="sub-environments"):
        model.set_env(_env(n=2))


def test_save_load_predict(emulated, tmp_path):
    env = _env(dim=7)
    model = sb.PPO2(MlpPolicy, env, n_steps=4, nminibatches=2, noptepochs=1, seed=5,
                    policy_kwargs={"net_arch": [dict(vf=[12, 9, 5], pi=[20])]}, cliprange_vf=-1, max_grad_norm=None)
    model.learn(total_timesteps=8)
    path = model.save(str(tmp_path / "ppo_model"))
    assert path.endswith(".zip") and not os.path.exists(str(tmp_path / "ppo_model.zip") + ".state")
    data, params = __import__("grasp_rl.sb.save_util", fromlist=["x"]).load_from_zip(path)
    assert list(params)[:6] == ["model/pi_fc0/w:0", "model/pi_fc0/b:0", "model/vf_fc0/w:0", "model/vf_fc0/b:0", "model/vf_fc1/w:0", "model/vf_fc1/b:0"]
    assert list(params)[-7:] == ["model/vf/w:0", "model/vf/b:0", "model/pi/w:0", "model/pi/b:0", "model/pi/logstd:0", "model/q/w:0", "model/q/b:0"]
    assert data["n_steps"] == 4 and data["cliprange_vf"] == -1 and data["max_grad_norm"] is None and data["gamma"] == 0.99
    loaded = sb.PPO2.load(path)
    assert loaded.get_env() is None and loaded.max_grad_norm is None and loaded.cliprange_vf == -1
    P, Q = model.get_parameters(), loaded.get_parameters()
    assert list(P) == list(Q) and all(np.array_equal(P[n], Q[n]) for n in P)
    obs = np.linspace(-1, 1, 7).astype(np.float32)
    a, state = model.predict(obs, deterministic=True)
    b, _ = loaded.predict(obs, deterministic=True)
    assert state is None and a.shape == (5,) and np.array_equal(a, b)
    batch, _ = loaded.predict(np.stack([obs, -obs, 0 * obs]), deterministic=True)       # more rows than environments
    assert batch.shape == (3, 5) and np.array_equal(batch[0], a)
    loaded.load_parameters({"model/pi/b:0": np.full(5, 7.0, np.float32)}, exact_match=False)
    c, _ = loaded.predict(obs, deterministic=True)
    assert np.array_equal(c, np.ones(5, np.float32))          # clipped to the space
    s1, _ = loaded.predict(obs)
    assert s1.shape == (5,) and (np.abs(s1) <= 1).all()
    with pytest.raises(Exception, match="parameter names do not match"):
        loaded.load_parameters({"model/pi/b:0": np.zeros(5, np.float32)})
    with pytest.raises(RuntimeError, match="unknown parameter"):
        loaded.load_parameters({"model/nope:0": np.zeros(1)}, exact_match=False)
    again = sb.PPO2.load(path, env=env)
    again.learn(total_timesteps=4)
    assert again.num_timesteps == 4


def test_what_is_refused_says_so(emulated, monkeypatch):
    env = _env()
    with pytest.raises(NotImplementedError, match="shared layers"):
        sb.PPO2(MlpPolicy, env, policy_kwargs={"net_arch": [64, dict(vf=[64], pi=[64])]})
    with pytest.raises(NotImplementedError, match="act_fun relu"):
        sb.PPO2(MlpPolicy, env, policy_kwargs={"act_fun": type("relu", (), {})})
    with pytest.raises(NotImplementedError, match="CnnPolicy"):
        sb.PPO2(CnnPolicy, env)
    with pytest.raises(NotImplementedError, match="MlpLstmPolicy"):
        sb.PPO2(type("MlpLstmPolicy", (), {}), env)
    disc = DummyVecEnv([lambda: FakeGraspEnv(vector_dim=11, discrete_actions=4)])
    with pytest.raises(NotImplementedError, match="Discrete"):
        sb.PPO2(MlpPolicy, disc)
    with pytest.raises(NotImplementedError, match="callable cliprange"):
        sb.PPO2(MlpPolicy, env, cliprange=lambda f: 0.2)
    with pytest.raises(NotImplementedError, match="callable cliprange"):
        sb.PPO2(MlpPolicy, env, cliprange_vf=lambda f: 0.2)
    with pytest.raises(NotImplementedError, match="data_parallel"):
        sb.PPO2(MlpPolicy, env, data_parallel="auto")
    with pytest.raises(NotImplementedError, match="pi tower"):
        sb.PPO2(MlpPolicy, env, policy_kwargs={"net_arch": [dict(vf=[64], pi=[2048])]})
    with pytest.raises(AssertionError, match="not a factor"):
        sb.PPO2(MlpPolicy, env, n_steps=10, nminibatches=4)
    with pytest.raises(NotImplementedError):
        sb.TRPO(None, env)


def test_image_observations_are_flattened_not_scaled(emulated):
    env = DummyVecEnv([lambda: FakeGraspEnv("depth", seed=0)])
    model = sb.PPO2(MlpPolicy, env, n_steps=4, nminibatches=2, noptepochs=1, seed=0)
    assert model.get_parameters()["model/pi_fc0/w:0"].shape == (8192, 64)
    obs = env.reset()
    a, _ = model.predict(obs[0], deterministic=True)
    P = model.get_parameters()
    h = np.tanh(obs[0].reshape(1, -1).astype(np.float64) @ P["model/pi_fc0/w:0"] + P["model/pi_fc0/b:0"])
    h = np.tanh(h @ P["model/pi_fc1/w:0"] + P["model/pi_fc1/b:0"])
    assert np.allclose(a, np.clip(h @ P["model/pi/w:0"] + P["model/pi/b:0"], -1, 1)[0], atol=1e-5)
    model.learn(total_timesteps=4)
    assert model.num_timesteps == 4
