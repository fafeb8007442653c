"""``TRPO`` -- the stable-baselines surface the reference drives with ``--algo TRPO`` (sb_helper.py:129-136, loader
train_stable_baselines.py:95-96) -- on the emulation build: constructor defaults, the learn loop's timestep and callback
accounting, the floor(T / 128) minibatch rule, seeded reproducibility, save / load with ``oldpi/*``, predict, flattened image
observations, and everything the class refuses by name."""
import inspect
import os

import numpy as np
import pytest

import stable_baselines as sb
from fake_env import FakeGraspEnv
from grasp_rl.engine import TrpoEngine
from grasp_rl.sb import save_util
from grasp_rl.sb.callbacks import BaseCallback
from grasp_rl.sb.trpo import TRPO
from hostemu_backend import NumpyHostBackend
from stable_baselines.bench import Monitor
from stable_baselines.common.policies import CnnPolicy, MlpPolicy
from stable_baselines.common.vec_env import DummyVecEnv


@pytest.fixture
def emulated(monkeypatch, hostemu_lib):
    monkeypatch.delenv("GRL_NUM_ENVS", raising=False)
    monkeypatch.delenv("GRL_DATA_PARALLEL", raising=False)
    monkeypatch.setattr(TRPO, "_engine_factory", staticmethod(
        lambda cfg, trpo, device: TrpoEngine(cfg, trpo, backend=NumpyHostBackend(), lib_path=hostemu_lib)))


class Recorder(BaseCallback):
    def __init__(self, stop_at=None):
        super().__init__()
        self.steps, self.starts, self.ends, self.stop_at, self.timesteps, self.order = 0, 0, 0, stop_at, [], []

    def _on_rollout_start(self):
        self.starts += 1
        self.order.append("start")

    def _on_rollout_end(self):
        self.ends += 1
        self.order.append("end")

    def _on_step(self):
        self.steps += 1
        if self.order[-1] != "step":
            self.order.append("step")
        self.timesteps.append(self.num_timesteps)
        assert self.locals["clipped_actions"].min() >= -1.0 and self.locals["clipped_actions"].max() <= 1.0
        return self.stop_at is None or self.steps < self.stop_at


def _env(n=1, dim=11, tmp=None, episode_len=5):
    def mk(k):
        e = FakeGraspEnv(vector_dim=dim, seed=k, episode_len=episode_len)
        return (lambda: Monitor(e, os.path.join(str(tmp), "log_%d" % k))) if tmp is not None else (lambda: e)
    return DummyVecEnv([mk(k) for k in range(n)])


def test_the_alias_is_the_real_class_with_the_defaults_of_stable_baselines(emulated):
    from grasp_rl import sb as gsb
    from stable_baselines.trpo_mpi import TRPO as aliased
    assert sb.TRPO is TRPO and gsb.TRPO is TRPO and aliased is TRPO
    d = {k: p.default for k, p in inspect.signature(TRPO.__init__).parameters.items() if p.default is not inspect.Parameter.empty}
    want = dict(gamma=0.99, timesteps_per_batch=1024, max_kl=0.01, cg_iters=10, lam=0.98, entcoeff=0.0, cg_damping=1e-2,
                vf_stepsize=3e-4, vf_iters=3, verbose=0, tensorboard_log=None, policy_kwargs=None, seed=None)
    assert {k: d[k] for k in want} == want
    model = sb.TRPO(MlpPolicy, _env(), timesteps_per_batch=400)
    t = model.engine.trpo
    assert (t.n_steps, t.cg_iters, t.ls_steps, t.fvp_stride, t.vf_batch) == (400, 10, 10, 5, 128)
    assert model.engine.cfg.act_batch == 1 and model.engine.cfg.batch_size == 128 and abs(model.engine.cfg.lr - 3e-4) < 1e-9
    assert model.n_vf_minibatches == 3 * 3      # floor(400 / 128) per iteration, 16 rows dropped
    assert sb.TRPO(MlpPolicy, _env(), timesteps_per_batch=127).n_vf_minibatches == 0
    assert sb.TRPO(MlpPolicy, _env(), timesteps_per_batch=256, vf_iters=2).n_vf_minibatches == 4


def test_learn_counts_steps_callbacks_and_resets(emulated, tmp_path):
    env = _env(tmp=tmp_path)
    model = sb.TRPO(MlpPolicy, env, timesteps_per_batch=130, seed=3, gamma=0.97, vf_stepsize=1e-3)
    p0 = model.get_parameters()
    assert [n for n in p0][:4] == ["model/pi_fc0/w:0", "model/pi_fc0/b:0", "model/vf_fc0/w:0", "model/vf_fc0/b:0"]
    rec = Recorder()
    model.learn(total_timesteps="131", callback=rec)      # runs until timesteps_so_far >= total: two batches of 130
    assert rec.steps == 260 and model.num_timesteps == 260 and rec.starts == 2 and rec.ends == 2
    assert rec.order == ["start", "step", "end", "start", "step", "end"]
    assert rec.timesteps[0] == 0 and rec.timesteps[129] == 0 and rec.timesteps[130] == 130      # per batch, as stable-baselines counts
    p1 = model.get_parameters()
    for n in p0:
        assert np.array_equal(p0[n], p1[n]) == n.startswith("model/q/"), n      # 130 >= 128: the value fit ran too
    assert all(np.isfinite(v).all() for v in p1.values())
    assert model.episodes_so_far == 52 and list(model.len_buffer)[:2] == [5, 5] and len(model.ep_info_buf) == 52
    # an episode end is followed by the generator's own reset, on top of the one the vec env made
    assert env.envs[0].env.n_resets == 1 + 2 * 52
    assert model.get_env().num_envs == 1 and model.get_vec_normalize_env() is None
    m = model.engine.metrics()
    assert m["ls_index"] >= -1 and (m["ls_index"] < 0 or m["trial_meankl"] <= 1.5 * 0.01)


def test_fewer_than_128_steps_train_no_value_variable(emulated):
    model = sb.TRPO(MlpPolicy, _env(), timesteps_per_batch=40, seed=1)
    p0 = model.get_parameters()
    model.learn(total_timesteps=40)
    p1 = model.get_parameters()
    for n in p0:
        assert np.array_equal(p0[n], p1[n]) == ("/pi" not in n), n


def test_same_seed_same_parameters_and_a_stop_from_on_step(emulated):
    P = []
    for _ in range(2):
        model = sb.TRPO(MlpPolicy, _env(), timesteps_per_batch=130, seed=11)
        model.learn(total_timesteps=130)
        P.append(model.get_parameters())
    assert all(np.array_equal(P[0][n], P[1][n]) for n in P[0])
    model = sb.TRPO(MlpPolicy, _env(), timesteps_per_batch=20, seed=11)
    rec = Recorder(stop_at=29)
    model.learn(total_timesteps=600, callback=rec)
    assert rec.steps == 29 and model.num_timesteps == 20      # one batch trained, the second abandoned
    model.learn(total_timesteps=20)                           # the slot the stop left open does not block the next run
    assert model.num_timesteps == 20


def test_logger_keys(emulated, capsys):
    model = sb.TRPO(MlpPolicy, _env(), timesteps_per_batch=20, seed=0, verbose=1)
    model.learn(total_timesteps=20)
    out = capsys.readouterr().out
    for key in ("EpLenMean", "EpRewMean", "EpThisIter", "EpisodesSoFar", "TimestepsSoFar", "TimeElapsed", "explained_variance_tdlam_before",
                "optimgain", "meankl", "entloss", "surrgain", "entropy"):
        assert key in out, key


def test_save_load_predict_with_oldpi(emulated, tmp_path):
    env = _env(dim=7)
    model = sb.TRPO(MlpPolicy, env, timesteps_per_batch=30, seed=5, policy_kwargs={"net_arch": [dict(vf=[12, 9, 5], pi=[20])]},
                    max_kl=0.02, vf_iters=2)
    first = model.save(str(tmp_path / "fresh"))
    _, params = save_util.load_from_zip(first)
    assert all(np.array_equal(params["oldpi/" + n[6:]], params[n]) for n in params if n.startswith("model/"))      # a copy before any update
    before = model.get_parameters()
    model.learn(total_timesteps=30)
    path = model.save(str(tmp_path / "trpo_model"))
    assert path.endswith(".zip")
    data, params = save_util.load_from_zip(path)
    names = list(params)
    half = len(names) // 2
    assert all(n.startswith("model/") for n in names[:half]) and names[half:] == ["oldpi/" + n[6:] for n in names[:half]]
    assert names[half - 7:half] == ["model/vf/w:0", "model/vf/b:0", "model/pi/w:0", "model/pi/b:0", "model/pi/logstd:0", "model/q/w:0", "model/q/b:0"]
    assert all(np.array_equal(params["oldpi/" + n[6:]], before[n]) for n in before)      # the snapshot at the start of the last update
    assert not np.array_equal(params["model/pi/w:0"], params["oldpi/pi/w:0"]) or model.engine.metrics()["ls_index"] < 0
    for k, v in dict(timesteps_per_batch=30, max_kl=0.02, vf_iters=2, gamma=0.99, lam=0.98, cg_iters=10, entcoeff=0.0, cg_damping=1e-2,
                     vf_stepsize=3e-4, using_gail=False, g_step=1, d_step=1, d_stepsize=3e-4, hidden_size_adversary=100,
                     adversary_entcoeff=1e-3, expert_dataset=None, n_envs=1, _vectorize_action=False).items():
        assert data[k] == v, k
    loaded = sb.TRPO.load(path)
    assert loaded.get_env() is None and loaded.max_kl == 0.02 and loaded.timesteps_per_batch == 30
    P, Q = model.get_parameters(), loaded.get_parameters()
    assert list(P) == list(Q) and all(np.array_equal(P[n], Q[n]) for n in P)
    obs = np.linspace(-1, 1, 7).astype(np.float32)
    a, state = model.predict(obs, deterministic=True)
    b, _ = loaded.predict(obs, deterministic=True)
    assert state is None and a.shape == (5,) and np.array_equal(a, b)
    batch, _ = loaded.predict(np.stack([obs, -obs, 0 * obs]), deterministic=True)
    assert batch.shape == (3, 5) and np.array_equal(batch[0], a)
    s1, _ = loaded.predict(obs)
    assert s1.shape == (5,) and (np.abs(s1) <= 1).all()
    # a zip without oldpi/*
    plain = save_util.save_to_zip(str(tmp_path / "plain"), data, model.get_parameters())
    again = sb.TRPO.load(plain, env=env)
    assert all(np.array_equal(P[n], again.get_parameters()[n]) for n in P)
    again.load_parameters(path)
    again.learn(total_timesteps=30)
    assert again.num_timesteps == 30


def test_what_is_refused_says_so(emulated, monkeypatch):
    env = _env()
    with pytest.raises(NotImplementedError, match="TRPO: policy None"):
        sb.TRPO(None, env)
    with pytest.raises(NotImplementedError, match="TRPO: shared layers"):
        sb.TRPO(MlpPolicy, env, policy_kwargs={"net_arch": [64, dict(vf=[64], pi=[64])]})
    with pytest.raises(NotImplementedError, match="TRPO: act_fun relu"):
        sb.TRPO(MlpPolicy, env, policy_kwargs={"act_fun": type("relu", (), {})})
    with pytest.raises(NotImplementedError, match="CnnPolicy"):
        sb.TRPO(CnnPolicy, env)
    with pytest.raises(NotImplementedError, match="MlpLstmPolicy"):
        sb.TRPO(type("MlpLstmPolicy", (), {}), env)
    with pytest.raises(NotImplementedError, match="TRPO: policy 'CnnPolicy'"):
        sb.TRPO("CnnPolicy", env)
    disc = DummyVecEnv([lambda: FakeGraspEnv(vector_dim=11, discrete_actions=4)])
    with pytest.raises(NotImplementedError, match="TRPO: Discrete"):
        sb.TRPO(MlpPolicy, disc)
    with pytest.raises(ValueError, match="the model requires a non vectorized environment or a single vectorized environment"):
        sb.TRPO(MlpPolicy, _env(n=2))
    monkeypatch.setenv("GRL_NUM_ENVS", "4")      # does not fan a TRPO env out
    assert sb.TRPO(MlpPolicy, _env(), timesteps_per_batch=8).get_env().num_envs == 1
    monkeypatch.delenv("GRL_NUM_ENVS")
    with pytest.raises(NotImplementedError, match="GAIL arguments .*expert_dataset"):
        sb.TRPO(MlpPolicy, env, expert_dataset=object())
    with pytest.raises(NotImplementedError, match="GAIL arguments .*using_gail"):
        sb.TRPO(MlpPolicy, env, using_gail=True)
    monkeypatch.setenv("GRL_DATA_PARALLEL", "auto")
    with pytest.raises(NotImplementedError, match="data_parallel"):
        sb.TRPO(MlpPolicy, env)
    monkeypatch.delenv("GRL_DATA_PARALLEL")
    with pytest.raises(NotImplementedError, match="cg_iters"):
        sb.TRPO(MlpPolicy, env, cg_iters=65)
    with pytest.raises(NotImplementedError, match="DDPG"):
        sb.DDPG(None, env)


def test_image_observations_are_flattened_not_scaled(emulated):
    env = DummyVecEnv([lambda: FakeGraspEnv("depth", seed=0)])
    model = sb.TRPO(MlpPolicy, env, timesteps_per_batch=6, seed=0)
    assert model.get_parameters()["model/pi_fc0/w:0"].shape == (8192, 64)
    obs = env.reset()
    a, _ = model.predict(obs[0], deterministic=True)
    P = model.get_parameters()
    h = np.tanh(obs[0].reshape(1, -1).astype(np.float64) @ P["model/pi_fc0/w:0"] + P["model/pi_fc0/b:0"])
    h = np.tanh(h @ P["model/pi_fc1/w:0"] + P["model/pi_fc1/b:0"])
    assert np.allclose(a, np.clip(h @ P["model/pi/w:0"] + P["model/pi/b:0"], -1, 1)[0], atol=1e-5)
    model.learn(total_timesteps=6)
    assert model.num_timesteps == 6
