"""``GAIL`` -- stable-baselines 2.10.1 ``gail/model.py`` over the TRPO class and a discriminator session of the engine -- on the
emulation build: construction and the aliases, the learn loop's timestep accounting and its log line, the loader's indices, the
discriminator update schedule, save / load through both classes, and everything the class refuses by name."""
import inspect
import os

import numpy as np
import pytest

import stable_baselines as sb
from fake_env import FakeGraspEnv
from grasp_rl.engine import TrpoEngine
from grasp_rl.sb import save_util
from grasp_rl.sb.expert import DataLoader, ExpertDataset, generate_expert_traj
from grasp_rl.sb.gail import GAIL
from grasp_rl.sb.trpo import TRPO
from hostemu_backend import NumpyHostBackend
from stable_baselines.common.policies import MlpPolicy
from stable_baselines.common.vec_env import DummyVecEnv

T = 16


@pytest.fixture
def emulated(monkeypatch, hostemu_lib):
    for k in ("GRL_NUM_ENVS", "GRL_DATA_PARALLEL", "GRL_CHECKPOINT_STATE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(TRPO, "_engine_factory", staticmethod(
        lambda cfg, trpo, device: TrpoEngine(cfg, trpo, backend=NumpyHostBackend(), lib_path=hostemu_lib)))


def _env(n=1, dim=11, **kw):
    return DummyVecEnv([(lambda k=k: FakeGraspEnv(vector_dim=dim, seed=k, episode_len=5, **kw)) for k in range(n)])


@pytest.fixture(scope="module")
def dataset():
    np.random.seed(0)
    env = FakeGraspEnv(vector_dim=11, seed=7, episode_len=5)
    data = generate_expert_traj(lambda obs: np.full(5, 0.25, np.float32) * np.sign(obs[0]), None, env, n_episodes=8)
    return ExpertDataset(traj_data=data, batch_size=8, verbose=0)


def _model(dataset, **kw):
    return sb.GAIL(MlpPolicy, _env(), dataset, timesteps_per_batch=T, g_step=2, d_step=3, hidden_size_adversary=12, seed=3, vf_iters=1,
                   policy_kwargs=dict(net_arch=[dict(pi=[8], vf=[8])]), **kw)


def test_the_aliases_are_the_class_and_the_defaults_are_those_of_stable_baselines(emulated, dataset):
    from stable_baselines.gail import GAIL as aliased
    assert sb.GAIL is GAIL and aliased is GAIL and sb.gail.GAIL is sb.GAIL and issubclass(GAIL, TRPO)
    d = {k: p.default for k, p in inspect.signature(GAIL.__init__).parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(expert_dataset=None, hidden_size_adversary=100, adversary_entcoeff=1e-3, g_step=3, d_step=1, d_stepsize=3e-4, verbose=0,
                     _init_setup_model=True)
    assert inspect.signature(GAIL.learn).parameters["tb_log_name"].default == "GAIL"
    m = _model(dataset)
    assert m.using_gail and m.d_batch == T // 3 and (m.g_step, m.d_step) == (2, 3)
    shapes = m.engine.gail_param_shapes()
    assert list(shapes.items()) == [("adversary/fully_connected/weights:0", (16, 12)), ("adversary/fully_connected/biases:0", (12,)),
                                    ("adversary/fully_connected_1/weights:0", (12, 12)), ("adversary/fully_connected_1/biases:0", (12,)),
                                    ("adversary/fully_connected_2/weights:0", (12, 1)), ("adversary/fully_connected_2/biases:0", (1,))]
    P = m.engine.gail_get_parameters()
    for n, p in P.items():      # seeded Glorot-uniform weights, zero biases
        if p.ndim == 2:
            lim = np.sqrt(6.0 / sum(p.shape))
            assert np.abs(p).max() <= lim and np.abs(p).max() > 0.5 * lim, n
        else:
            assert not p.any(), n
    P2 = _model(dataset).engine.gail_get_parameters()
    assert all(np.array_equal(P[n], P2[n]) for n in P)


def test_the_loader_hands_out_the_indices_of_its_next_batch_from_the_same_draws():
    obs, act = np.arange(22, dtype=np.float32).reshape(11, 2), np.arange(11, dtype=np.float32).reshape(11, 1)
    a, b = DataLoader(np.arange(11), obs, act, 4), DataLoader(np.arange(11), obs, act, 4)
    np.random.seed(5)
    batches = [next(a) for _ in range(7)]
    np.random.seed(5)
    rows = [b.next_indices() for _ in range(7)]
    assert [len(r) for r in rows] == [4, 4, 3, 4, 4, 3, 4]
    for (o, ac), r in zip(batches, rows):
        assert np.array_equal(o, obs[r]) and np.array_equal(ac, act[r])
    np.random.seed(5)
    c = DataLoader(np.arange(11), obs, act, 4)      # the two calls share one cursor
    assert np.array_equal(next(c)[0], batches[0][0]) and np.array_equal(c.next_indices(), rows[1]) and np.array_equal(next(c)[0], batches[2][0])


def test_learn_counts_timesteps_as_trpo_and_logs_true_returns_and_the_six_losses(emulated, dataset, capsys):
    m = _model(dataset, verbose=1)
    calls = []
    upd, rew = m.engine.gail_update, m.engine.gail_rewards
    m.engine.gail_update = lambda table, g, e: (calls.append(("update", g.copy(), e.copy())), upd(table, g, e))[1]
    m.engine.gail_rewards = lambda: (calls.append(("rewards",)), rew())[1]
    P0 = m.engine.gail_get_parameters()
    m.learn(2 * T * 2)      # g_step x T x 2 steps: four rollouts, two discriminator updates
    assert m.num_timesteps == 4 * T
    assert [c[0] for c in calls] == ["rewards", "rewards", "update", "rewards", "rewards", "update"]
    b = T // 3
    for _, g, e in (c for c in calls if c[0] == "update"):
        assert g.shape == e.shape == (T // b, b) and len(set(g.reshape(-1))) == g.size and g.min() >= 0 and g.max() < T
        assert e.min() >= -1 and e.max() < dataset.observations.shape[0]
    out = capsys.readouterr().out
    for key in ("EpRewMean", "EpTrueRewMean", "generator_loss", "expert_loss", "entropy", "entropy_loss", "generator_acc", "expert_acc",
                "TimestepsSoFar"):
        assert key in out, key
    assert m.last_d_losses.shape == (6,) and np.isfinite(m.last_d_losses).all()
    assert abs(m.last_d_losses[3] + 1e-3 * m.last_d_losses[2]) < 1e-6
    # the discriminator rewards are positive; the environment's returns are what FakeGraspEnv pays
    assert min(m.rew_buffer) > 0 and len(m.true_rew_buffer) == len(m.rew_buffer)
    P1 = m.engine.gail_get_parameters()
    assert all(not np.array_equal(P0[n], P1[n]) for n in P0)
    s, q, n = m.engine.gail_get_stats()
    assert n == 1e-2 + sum((e >= 0).sum() + g.size for _, g, e in (c for c in calls if c[0] == "update"))


def test_save_and_load_through_both_classes_predict_identically_and_the_zip_holds_no_dataset(emulated, dataset, tmp_path, monkeypatch):
    m = _model(dataset)
    m.learn(T)
    path = str(tmp_path / "gail.zip")
    m.save(path)
    assert sorted(os.listdir(str(tmp_path))) == ["gail.zip"]
    data, params = save_util.load_from_zip(path)
    assert data["using_gail"] is True and data["expert_dataset"] is None and (data["g_step"], data["d_step"]) == (2, 3)
    assert data["hidden_size_adversary"] == 12 and not any(n.startswith("adversary") for n in params)
    assert m.expert_dataset is dataset
    obs = np.random.default_rng(0).uniform(-1, 1, (6, 11)).astype(np.float32)
    want = m.predict(obs, deterministic=True)[0]
    g = sb.GAIL.load(path, _env(), expert_dataset=dataset)
    t = sb.TRPO.load(path, _env())
    assert type(g) is GAIL and type(t) is TRPO and g.expert_dataset is dataset and g.using_gail
    assert np.array_equal(g.predict(obs, deterministic=True)[0], want) and np.array_equal(t.predict(obs, deterministic=True)[0], want)
    g.learn(T)      # a loaded model starts a fresh adversary and learns on
    assert g.num_timesteps == T
    with pytest.raises(ValueError, match="learn needs an expert dataset"):
        sb.GAIL.load(path, _env()).learn(T)
    # a session is not in a checkpoint
    monkeypatch.setenv("GRL_CHECKPOINT_STATE", "1")
    m.save(str(tmp_path / "again.zip"))
    assert sorted(os.listdir(str(tmp_path))) == ["again.zip", "gail.zip"]
    with pytest.raises(NotImplementedError, match="GAIL: save_checkpoint is not implemented"):
        m.save_checkpoint(str(tmp_path / "ck.zip"))
    with pytest.raises(NotImplementedError, match="GAIL: load_checkpoint is not implemented"):
        sb.GAIL.load_checkpoint(path, _env())


def test_refusals_by_name(emulated, dataset):
    with pytest.raises(ValueError, match="learn needs an expert dataset"):
        sb.GAIL(MlpPolicy, _env(), timesteps_per_batch=T).learn(T)
    with pytest.raises(NotImplementedError, match="GAIL: Discrete action spaces are not implemented"):
        sb.GAIL(MlpPolicy, _env(discrete_actions=4), dataset, timesteps_per_batch=T)
    with pytest.raises(ValueError, match="non vectorized environment or a single vectorized environment"):
        sb.GAIL(MlpPolicy, _env(n=2), dataset, timesteps_per_batch=T)
    with pytest.raises(ValueError, match="observations of 11 and actions of 5 values, the spaces 9 and 5"):
        sb.GAIL(MlpPolicy, _env(dim=9), dataset, timesteps_per_batch=T).learn(T)
    with pytest.raises(ValueError, match="observations of 11 and actions of 5 values, the spaces 11 and 3"):
        sb.GAIL(MlpPolicy, _env(act_dim=3), dataset, timesteps_per_batch=T).learn(T)
    with pytest.raises(TypeError, match="unexpected keyword arguments \\['using_gail'\\]"):
        sb.GAIL(MlpPolicy, _env(), dataset, using_gail=True)
    with pytest.raises(NotImplementedError, match="hidden_size_adversary must be 1..1024"):
        sb.GAIL(MlpPolicy, _env(), dataset, hidden_size_adversary=2000)
    with pytest.raises(NotImplementedError, match="d_step 1..timesteps_per_batch"):
        sb.GAIL(MlpPolicy, _env(), dataset, timesteps_per_batch=T, d_step=T + 1)
    with pytest.raises(NotImplementedError, match="CnnPolicy"):
        from stable_baselines.common.policies import CnnPolicy
        sb.GAIL(CnnPolicy, _env(), dataset, timesteps_per_batch=T)
    with pytest.raises(NotImplementedError, match="the GAIL arguments"):      # (already pinned by tests/test_trpo_host.py)
        sb.TRPO(MlpPolicy, _env(), using_gail=True)
