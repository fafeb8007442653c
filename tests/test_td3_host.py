"""``TD3`` through the ``stable_baselines`` alias package on the g++ emulation build (no GPU): construction, the learn loop's update
rule, the zip round trip, N environments, VecNormalize statistics, and every refusal by its text."""
import functools
import os

import numpy as np
import pytest

import stable_baselines as sb
import td3_util as tu
from fake_env import FakeGraspEnv
from grasp_rl.engine import Td3Engine
from grasp_rl.sb.base import BaseModel
from grasp_rl.sb.td3 import TD3
from hostemu_backend import NumpyHostBackend
from stable_baselines.common.callbacks import BaseCallback
from stable_baselines.common.noise import NormalActionNoise
from stable_baselines.common.vec_env import DummyVecEnv, VecNormalize
from stable_baselines.td3.policies import CnnPolicy, LnMlpPolicy, MlpPolicy

OBS, ACT = 9, 3


def make_env(seed=0, **kw):
    return FakeGraspEnv(vector_dim=OBS, act_dim=ACT, seed=seed, **kw)


@pytest.fixture
def emu(hostemu_lib, monkeypatch):
    for k in ("GRL_NUM_ENVS", "GRL_DATA_PARALLEL", "GRL_CHECKPOINT_STATE", "GRL_DEVICE_NORM", "GRL_TUNE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(TD3, "_engine_factory",
                        staticmethod(lambda cfg, td3, device: Td3Engine(cfg, td3, backend=NumpyHostBackend(), lib_path=hostemu_lib)))


class Noise(NormalActionNoise):
    resets = 0

    def reset(self):
        self.resets += 1


class Spy(BaseCallback):
    def __init__(self):
        super().__init__()
        self.steps, self.dones = 0, 0

    def _on_step(self):
        self.steps += 1
        self.dones += int(np.sum(self.locals["done"]))
        return True


def _spy_train(model):
    calls, real = [], model.engine.train

    def train(n_updates=1, idx=None, eps=None, first_step=0):
        real(n_updates, idx, eps, first_step)
        calls.append((int(n_updates), int(first_step), model.engine.metrics()[:, 5].copy()))
    model.engine.train = train
    return calls


def test_both_policy_spellings_construct_a_model(emu):
    assert sb.TD3 is TD3 and issubclass(TD3, BaseModel) and sb.td3.MlpPolicy is MlpPolicy
    for policy in ("MlpPolicy", MlpPolicy):
        model = sb.TD3(policy, DummyVecEnv([make_env]), policy_kwargs={"layers": [16, 8]})
        assert list(model.get_parameters()) == tu.param_names(2)
        assert model.get_parameters()["model/values_fn/qf1/fc0/kernel:0"].shape == (OBS + ACT, 16)
        P = model.get_parameters()
        assert all(np.array_equal(P[n], P["model/" + n[len("target/"):]]) for n in P if n.startswith("target/"))
        assert (model.gamma, model.learning_rate, model.buffer_size, model.learning_starts, model.train_freq, model.gradient_steps,
                model.batch_size, model.tau, model.policy_delay, model.action_noise, model.target_policy_noise, model.target_noise_clip,
                model.random_exploration) == (0.99, 3e-4, 50000, 100, 100, 100, 128, 0.005, 2, None, 0.2, 0.5, 0.0)
        model.engine.close()


def test_learn_follows_stable_baselines_update_rule(emu):
    noise = Noise(np.zeros(ACT), 0.1 * np.ones(ACT))
    model = sb.TD3("MlpPolicy", DummyVecEnv([functools.partial(make_env, episode_len=7)]), buffer_size=500, learning_starts=20, train_freq=4,
                   gradient_steps=4, batch_size=32, policy_delay=3, action_noise=noise, policy_kwargs={"layers": [16]}, seed=3,
                   learning_rate=lambda frac: 1e-3 * frac)
    calls, spy = _spy_train(model), Spy()
    p0 = model.get_parameters()
    model.learn(300, callback=spy)
    # step s (0-based) trains iff s % train_freq == 0, the replay (s + 1 rows) can fill a batch and num_timesteps (s + 1) has
    # reached learning_starts: all gradient_steps updates of that step or -- the loop's break -- none
    want = [s for s in range(300) if s % 4 == 0 and s + 1 >= 32 and s + 1 >= 20]
    assert [(n, f) for n, f, _ in calls] == [(4, s) for s in want]
    assert model.n_updates == 4 * len(want) and model.num_timesteps == 300 and spy.steps == 300
    for n, first, flags in calls:      # a policy update happens when (step + grad_step) % policy_delay == 0
        assert list(flags) == [1.0 if (first + g) % 3 == 0 else 0.0 for g in range(n)]
    assert noise.resets == 1 + spy.dones and spy.dones == 300 // 7      # learn's own reset, then one per episode end
    p1 = model.get_parameters()
    assert all(not np.array_equal(p0[n], p1[n]) for n in p0)
    assert model.engine.adam_steps() == (4 * len(want), sum(int(f.sum()) for _, _, f in calls))
    m = model.engine.metrics()
    assert m.shape == (4, 6) and np.isfinite(m).all()
    model.engine.close()


def test_save_load_round_trip(emu, tmp_path):
    env = DummyVecEnv([make_env])
    noise = NormalActionNoise(np.zeros(ACT), 0.3 * np.ones(ACT))
    model = sb.TD3("MlpPolicy", env, learning_starts=4, train_freq=1, gradient_steps=2, batch_size=8, policy_delay=2, tau=0.01,
                   target_policy_noise=0.3, target_noise_clip=0.6, action_noise=noise, policy_kwargs={"layers": [12, 10]}, seed=1)
    model.learn(30)
    path = str(tmp_path / "td3_model")
    model.save(path)
    loaded = sb.TD3.load(path, action_noise=noise)      # (keyword overrides as stable-baselines' load takes them)
    P, Q = model.get_parameters(), loaded.get_parameters()
    assert list(P) == list(Q) == tu.param_names(2)      # model/* then target/*, TF creation order
    assert all(tu.same_bits(P[n], Q[n]) for n in P)
    assert (loaded.policy_delay, loaded.tau, loaded.target_policy_noise, loaded.target_noise_clip, loaded.batch_size,
            loaded.gradient_steps, loaded.policy_kwargs) == (2, 0.01, 0.3, 0.6, 8, 2, {"layers": [12, 10]})
    obs = env.reset()
    a, _ = loaded.predict(obs, deterministic=True)
    assert a.shape == (1, ACT) and np.array_equal(a, loaded.predict(obs)[0]) and np.array_equal(a, model.predict(obs)[0])
    np.random.seed(0)
    noisy = np.stack([loaded.predict(obs, deterministic=False)[0] for _ in range(50)])
    assert noisy.std(axis=0).min() > 0.01      # the noise is drawn anew per call
    assert np.all(noisy >= env.action_space.low) and np.all(noisy <= env.action_space.high)
    loaded.action_noise = None
    assert np.array_equal(loaded.predict(obs, deterministic=False)[0], a)      # without noise: the policy's action either way
    # load_parameters with a subset
    sub = {n: np.zeros_like(P[n]) for n in ("model/pi/dense/kernel:0", "model/pi/dense/bias:0")}
    loaded.load_parameters(sub, exact_match=False)
    assert not loaded.predict(obs)[0].any()
    with pytest.raises(Exception, match="parameter names do not match"):
        loaded.load_parameters(sub, exact_match=True)
    with pytest.raises(RuntimeError, match="unknown parameter"):
        loaded.load_parameters({"model/vf/w:0": np.zeros(1)}, exact_match=False)
    model.engine.close()
    loaded.engine.close()


def test_four_environments_fan_out(emu, monkeypatch):
    monkeypatch.setenv("GRL_NUM_ENVS", "4")
    monkeypatch.setenv("GRL_ENV_START_METHOD", "fork")      # (the emulation engine has no HIP context a fork could damage)
    # forked workers inherit this process's module state: an encoder record left HERE (as other tests of a whole-suite run leave
    # them) is not one the workers deferred, and the fan-out must not take it for one
    from grasp_rl import autoencoder
    stale = autoencoder.DeferredEncoder(None)
    assert stale._record in autoencoder._DEFERRED and autoencoder.deferred_records()
    env = DummyVecEnv([functools.partial(make_env, None)])
    model = None
    try:
        model = sb.TD3("MlpPolicy", env, learning_starts=8, train_freq=2, gradient_steps=3, batch_size=16, policy_kwargs={"layers": [8]})
        assert model.n_envs == 4 and model.engine.cfg.act_batch == 4 and model.get_env().num_envs == 4
        calls, spy = _spy_train(model), Spy()
        model.learn(80, callback=spy)
        assert model.num_timesteps == 80 and spy.steps == 20 and model.engine.replay_size() == 80
        assert [(n, f) for n, f, _ in calls] == [(3, s) for s in range(20) if s % 2 == 0 and 4 * (s + 1) >= 16]
        a, _ = model.predict(np.zeros((4, OBS), np.float32))
        assert a.shape == (4, ACT)
    finally:
        autoencoder._DEFERRED.remove(stale._record)
        if model is not None:
            model.get_env().close()
            model.engine.close()
        env.close()


def test_vec_normalize_statistics_reach_the_engine_before_an_update(emu):
    env = VecNormalize(DummyVecEnv([make_env]), norm_obs=True, norm_reward=True, clip_obs=5.0)
    model = sb.TD3("MlpPolicy", env, learning_starts=4, train_freq=1, gradient_steps=1, batch_size=4, policy_kwargs={"layers": [8]})
    assert model.engine.cfg.normalize == 1 and model.engine.cfg.clip_obs == 5.0
    pushed, order = [], []
    real_set, real_train = model.engine.set_obs_stats, model.engine.train

    def set_obs_stats(mean, var, ret_var):
        pushed.append((np.array(mean, copy=True), float(env.obs_rms.count)))
        order.append("stats")
        return real_set(mean, var, ret_var)

    def train(*a, **k):
        order.append("train")
        assert pushed and pushed[-1][1] == float(env.obs_rms.count) and np.array_equal(pushed[-1][0], env.obs_rms.mean)
        return real_train(*a, **k)
    model.engine.set_obs_stats, model.engine.train = set_obs_stats, train
    model.learn(12)
    assert order.count("train") == 9 and order[:2] == ["stats", "train"] and order.count("stats") == 9
    # the replay holds RAW observations and rewards: normalised at sample time
    raw = model.engine.fetch("rp_obs", (model.buffer_size, OBS))[:12]
    assert np.all(np.abs(raw) <= 1.0) and np.abs(model.engine.fetch("rp_rew", (model.buffer_size,))[:12]).min() > 50.0
    env.training = False
    model.engine.train(2, first_step=0)
    assert order[-1] == "train"
    model.engine.close()


def test_refusals_by_their_text(emu, tmp_path, monkeypatch):
    env = DummyVecEnv([make_env])
    for policy, kw, text in (("CnnPolicy", {}, "TD3: CnnPolicy is not implemented"), (CnnPolicy, {}, "TD3: CnnPolicy is not implemented"),
                             ("LnMlpPolicy", {}, "TD3: LnMlpPolicy is not implemented"), (LnMlpPolicy, {}, "TD3: LnMlpPolicy is not implemented"),
                             ("MlpPolicy", {"layer_norm": True}, "TD3: layer_norm is not implemented"),
                             ("MlpPolicy", {"feature_extraction": "cnn"}, "TD3: CnnPolicy is not implemented")):
        with pytest.raises(NotImplementedError, match=text):
            sb.TD3(policy, env, policy_kwargs=kw)
    with pytest.raises(NotImplementedError, match="TD3: a non-Box action space is not implemented"):
        sb.TD3("MlpPolicy", DummyVecEnv([functools.partial(make_env, discrete_actions=4)]))
    with pytest.raises(NotImplementedError, match="TD3: data_parallel is not implemented"):
        sb.TD3("MlpPolicy", env, data_parallel="auto")
    with pytest.raises(NotImplementedError, match="TD3: device_norm=True is not implemented"):
        sb.TD3("MlpPolicy", env, device_norm=True)
    model = sb.TD3("MlpPolicy", env, policy_kwargs={"layers": [8]})
    with pytest.raises(NotImplementedError, match="TD3: save_checkpoint is not implemented"):
        model.save_checkpoint(str(tmp_path / "ck"))
    with pytest.raises(NotImplementedError, match="TD3: load_checkpoint is not implemented"):
        sb.TD3.load_checkpoint(str(tmp_path / "ck"))
    with pytest.raises(NotImplementedError, match="TD3: pretrain is not implemented"):
        model.pretrain(None)
    monkeypatch.setenv("GRL_CHECKPOINT_STATE", "1")
    with pytest.raises(NotImplementedError, match="TD3: save_checkpoint is not implemented"):
        model.save(str(tmp_path / "m"))
    assert not os.listdir(tmp_path)
    model.engine.close()
    with pytest.raises(NotImplementedError, match="DDPG is outside the accelerated hot path"):      # DDPG stays refused as it is
        sb.DDPG("MlpPolicy", env)
