"""The stable-baselines surface of behaviour-cloning pretraining on the emulated engine: generate_expert_traj and ExpertDataset
(``stable_baselines.gail``), ``SAC.pretrain`` with its printed losses held to the float64 restatement of tests/bc_util.py, and
what is refused by name."""
import numpy as np
import pytest

import bc_util as bu
from fake_env import FakeGraspEnv
from grasp_rl.engine import SacEngine
from grasp_rl.sb.dqn import BDQ, DQN
from grasp_rl.sb.sac import SAC
from grasp_rl.sb.spaces import Box
from hostemu_backend import NumpyHostBackend
from oracle import sac as osac
from stable_baselines import PPO2, TRPO
from stable_baselines.common.vec_env import DummyVecEnv
from stable_baselines.gail import ExpertDataset, generate_expert_traj
from stable_baselines.sac.policies import MlpPolicy


@pytest.fixture
def emulated(hostemu_lib, monkeypatch):
    monkeypatch.delenv("GRL_NUM_ENVS", raising=False)
    monkeypatch.delenv("GRL_DATA_PARALLEL", raising=False)
    monkeypatch.setattr(SAC, "_engine_factory",
                        staticmethod(lambda cfg, device: SacEngine(cfg, backend=NumpyHostBackend(), lib_path=hostemu_lib)))


def _record(tmp_path, n_episodes=6, episode_len=7, dim=11, env=None):
    env = env or FakeGraspEnv(vector_dim=dim, seed=3, episode_len=episode_len)
    rng = np.random.default_rng(5)
    path = str(tmp_path / "expert")
    data = generate_expert_traj(lambda obs: rng.uniform(-1, 1, 5).astype(np.float32), path, env, n_episodes=n_episodes)
    return path + ".npz", data


def test_generate_expert_traj_writes_the_five_keys_and_the_dataset_reads_them_back(tmp_path, capsys):
    path, data = _record(tmp_path)
    z = np.load(path)
    assert sorted(z.files) == sorted(("actions", "obs", "rewards", "episode_returns", "episode_starts"))
    assert z["obs"].shape == (42, 11) and z["actions"].shape == (42, 5) and z["rewards"].shape == (42,)
    assert z["episode_starts"].shape == (42,) and z["episode_returns"].shape == (6,)
    assert list(np.flatnonzero(z["episode_starts"])) == list(range(0, 42, 7))
    assert np.allclose(z["episode_returns"], z["rewards"].reshape(6, 7).sum(1))
    for k in z.files:
        assert np.array_equal(z[k], data[k])
    ds = ExpertDataset(expert_path=path, batch_size=8, verbose=1)
    assert "Total trajectories: 6" in capsys.readouterr().out
    assert ds.observations.shape == (42, 11) and ds.observations.dtype == np.float32 and ds.num_transition == 42
    assert sorted(np.concatenate([ds.train_indices, ds.val_indices])) == list(range(42))
    obs, act = ds.get_next_batch("train")
    assert obs.shape == (8, 11) and act.shape == (8, 5)
    ds.init_dataloader(5)
    assert ds.get_next_batch()[0].shape == (5, 11)


def test_a_vectorised_env_of_one_records_the_same_arrays(tmp_path):
    venv = DummyVecEnv([lambda: FakeGraspEnv(vector_dim=11, seed=3, episode_len=7)])
    rng = np.random.default_rng(5)
    data = generate_expert_traj(lambda obs: rng.uniform(-1, 1, (1, 5)).astype(np.float32), None, venv, n_episodes=6)
    _, ref = _record(tmp_path)
    for k in ref:
        assert np.array_equal(data[k], ref[k]), k


@pytest.mark.parametrize("fraction,limit,batch,n_train,n_val,n_mb", [
    (0.7, -1, 8, 29, 13, 4),          # 29 = 3 * 8 + 5: a partial minibatch
    (0.5, -1, 7, 21, 21, 3),          # whole minibatches only
    (0.7, 2, 4, 9, 5, 3),             # two episodes of seven steps
])
def test_split_sizes_and_minibatch_counts(tmp_path, fraction, limit, batch, n_train, n_val, n_mb):
    _, data = _record(tmp_path)
    ds = ExpertDataset(traj_data=data, train_fraction=fraction, batch_size=batch, traj_limitation=limit, verbose=0)
    assert (len(ds.train_indices), len(ds.val_indices), len(ds.train_loader)) == (n_train, n_val, n_mb)
    rows = ds.train_loader.index_rows()
    assert rows.shape == (n_mb, batch) and rows.dtype == np.int32
    assert sorted(rows[rows >= 0]) == sorted(ds.train_indices) and (rows.reshape(-1)[n_train:] == -1).all()
    again = ds.train_loader.index_rows()
    assert sorted(again[again >= 0]) == sorted(rows[rows >= 0]) and not np.array_equal(again, rows)       # a fresh shuffle per epoch
    fixed = ExpertDataset(traj_data=data, train_fraction=fraction, batch_size=batch, traj_limitation=limit, verbose=0, randomize=False)
    assert np.array_equal(fixed.train_loader.index_rows(), fixed.train_loader.index_rows())
    if limit > 0:
        assert ds.num_traj == limit and ds.num_transition == 7 * limit
    with pytest.raises(ValueError, match="validation set"):
        ExpertDataset(traj_data=data, train_fraction=1.0, verbose=0)
    with pytest.raises(ValueError, match="training set"):
        ExpertDataset(traj_data=data, train_fraction=0.0, verbose=0)


def test_pretrain_returns_the_model_and_prints_the_restatements_losses(emulated, tmp_path, capsys):
    _, data = _record(tmp_path)
    env = FakeGraspEnv(vector_dim=11, seed=0)
    model = SAC(MlpPolicy, env, batch_size=16, buffer_size=100, verbose=1, seed=1)
    ds = ExpertDataset(traj_data=data, batch_size=8, verbose=0, randomize=False)
    P0 = model.get_parameters()
    steps, updates = model.num_timesteps, model.n_updates
    capsys.readouterr()
    assert model.pretrain(ds, n_epochs=4, learning_rate=1e-3, val_interval=2) is model
    out = capsys.readouterr().out
    assert (model.num_timesteps, model.n_updates) == (steps, updates)
    assert out.count("Training loss:") == 2 and "Epoch 2\n" in out and "Epoch 4\n" in out and "Epoch 3" not in out
    assert "==== Training progress 50.00% ====" in out and out.rstrip().endswith("Pretraining done.")
    # the restatement over the same minibatches (randomize=False: the loader's order is the split's)
    spec = osac.SacSpec(extractor="mlp", obs_dim=11, act_dim=5, layers=[64, 64])
    case = {"spec": spec, "bc_obs": ds.observations, "bc_act": ds.actions, "low": env.action_space.low, "high": env.action_space.high}
    names = bu.trained_names(spec)
    P, st = {n: v.copy() for n, v in P0.items()}, bu.adam_state0(P0, names)
    printed = [tuple(float(x.rstrip(",")) for x in l.split()[2::3]) for l in out.splitlines() if l.startswith("Training loss:")]
    k = 0
    for epoch in range(4):
        losses = []
        for row in ds.train_loader.index_rows():
            _, loss, G = bu.reference_update(case, P, row)
            losses.append(loss)
            osac.adam_apply(P, {n: G[n].astype(np.float32) for n in names}, st, 1e-3)
        if epoch % 2 == 1:
            val = np.mean([bu.reference_loss(case, P, row) for row in ds.val_loader.index_rows()])
            assert abs(printed[k][0] - np.mean(losses)) <= 2e-6 + 1e-3 * np.mean(losses), (printed[k], np.mean(losses))
            assert abs(printed[k][1] - val) <= 2e-6 + 1e-3 * val, (printed[k], val)
            k += 1
    P1 = model.get_parameters()
    for n in P1:
        assert np.array_equal(P1[n], P0[n]) == (n not in names), n
    # verbose 0 prints nothing and trains the same
    quiet = SAC(MlpPolicy, env, batch_size=16, buffer_size=100, verbose=0, seed=1)
    quiet.pretrain(ds, n_epochs=4, learning_rate=1e-3, val_interval=2)
    assert capsys.readouterr().out == ""
    assert all(np.array_equal(v, P1[n]) for n, v in quiet.get_parameters().items())


def test_val_interval_default(emulated, tmp_path, capsys):
    _, data = _record(tmp_path)
    model = SAC(MlpPolicy, FakeGraspEnv(vector_dim=11, seed=0), batch_size=16, buffer_size=100, verbose=1, seed=1)
    ds = ExpertDataset(traj_data=data, batch_size=16, verbose=0)
    capsys.readouterr()
    model.pretrain(ds, n_epochs=3)
    assert capsys.readouterr().out.count("Validation loss:") == 3          # below ten epochs: every epoch
    model.pretrain(ds, n_epochs=20)
    assert capsys.readouterr().out.count("Validation loss:") == 10         # else every n_epochs // 10


def test_what_is_refused_says_so(emulated, tmp_path, monkeypatch):
    _, data = _record(tmp_path)
    env = FakeGraspEnv(vector_dim=11, seed=0)
    model = SAC(MlpPolicy, env, batch_size=8, buffer_size=100, seed=1)
    P0 = model.get_parameters()
    with pytest.raises(ValueError, match=r"dataset.batch_size \(16\) <= the model's batch_size \(8\)"):
        model.pretrain(ExpertDataset(traj_data=data, batch_size=16, verbose=0))
    other = dict(data, obs=data["obs"][:, :7])
    with pytest.raises(ValueError, match="observations of 7 and actions of 5 values, the model takes 11 and 5"):
        model.pretrain(ExpertDataset(traj_data=other, batch_size=8, verbose=0))
    model._dp_rt = object()            # one replica of a data-parallel job
    with pytest.raises(NotImplementedError, match="SAC: pretrain is not implemented under data parallelism"):
        model.pretrain(ExpertDataset(traj_data=data, batch_size=8, verbose=0))
    assert all(np.array_equal(v, P0[n]) for n, v in model.get_parameters().items())
    for cls in (DQN, BDQ, PPO2, TRPO):
        with pytest.raises(NotImplementedError, match="%s: pretrain is not implemented" % cls.__name__):
            cls.__new__(cls).pretrain(None)
    paths = dict(data, obs=np.array(["img_%d.png" % i for i in range(len(data["obs"]))]))
    with pytest.raises(NotImplementedError, match="ExpertDataset: image paths"):
        ExpertDataset(traj_data=paths, verbose=0)
    with pytest.raises(NotImplementedError, match="generate_expert_traj: image_folder is not implemented"):
        generate_expert_traj(lambda o: np.zeros(5, np.float32), None, env, n_episodes=1, image_folder="frames")
    with pytest.raises(ValueError, match="both"):
        ExpertDataset(expert_path="x.npz", traj_data=data)
    unbounded = SAC(MlpPolicy, env, batch_size=8, buffer_size=100, seed=1)
    unbounded.action_space = Box(-np.inf, np.inf, shape=(5,))
    with pytest.raises(Exception, match="action bounds must be finite"):
        unbounded.pretrain(ExpertDataset(traj_data=data, batch_size=8, verbose=0))
