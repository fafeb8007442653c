"""``DQN`` / ``BDQ`` with an MLP policy on IMAGE observations (what ``train_stable_baselines.py train --algo DQN`` builds on
config/gripper_grasp.yaml: ``sb.DQN(DQNMlpPolicy, env, ...)`` over a ``Box(0, 255, (64, 64, 2))``), on the emulation build:
the observation is flattened in C order and not divided by 255, the first kernel is [8192, H], and learn / predict / save /
load / load_parameters / checkpoint / VecNormalize on host and device all take the image as it comes."""
import numpy as np
import pytest

import q_device_norm_learn_util as dl
import q_layer_norm_util as ql
from fake_env import FakeGraspEnv
from grasp_rl.engine import QEngine
from grasp_rl.sb.dqn import BDQ, DQN
from grasp_rl.sb.vec_env import DummyVecEnv, VecNormalize
from hostemu_backend import NumpyHostBackend
from oracle import dqn as od
from stable_baselines.bdq.policies import MlpActPolicy
from stable_baselines.deepq.policies import CnnPolicy, LnMlpPolicy, MlpPolicy

SHAPE = (64, 64, 2)
OBS_DIM = 64 * 64 * 2


@pytest.fixture(autouse=True)
def emulation(hostemu_lib, monkeypatch):
    factory = staticmethod(lambda cfg, device: QEngine(cfg, backend=NumpyHostBackend(), lib_path=hostemu_lib))
    monkeypatch.setattr(DQN, "_engine_factory", factory, raising=False)
    monkeypatch.setattr(BDQ, "_engine_factory", factory, raising=False)
    for k in ("GRL_DEVICE_NORM", "GRL_NUM_ENVS", "GRL_CHECKPOINT_STATE"):
        monkeypatch.delenv(k, raising=False)


def make_env(algo, normalize, n=1, seed=0):
    mk = lambda s: FakeGraspEnv(kind="depth", discrete_actions=6 if algo == "dqn" else None, seed=s)
    env = DummyVecEnv([(lambda s=s: mk(seed + s)) for s in range(n)])
    return VecNormalize(env, norm_obs=True, norm_reward=True, clip_obs=10.0) if normalize else env


def make_model(algo, env, **kw):
    kw = dict(dict(batch_size=8, learning_starts=12, buffer_size=64, seed=0, target_network_update_freq=16), **kw)
    if algo == "dqn":
        return DQN(MlpPolicy, env, **kw)
    return BDQ(MlpActPolicy, env, policy_kwargs={"layers": [[64, 64], [32], [32]]}, num_actions_pad=9, **kw)


def first_kernel(model):
    scope = "deepq/model/action_value" if model.algo == "dqn" else "bdq/model/common_net"
    return scope + "/fully_connected/weights:0"


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("algo", ["dqn", "bdq"])
def test_constructs_learns_predicts_saves_and_loads(algo, normalize, tmp_path):
    env = make_env(algo, normalize)
    model = make_model(algo, env)
    assert model.engine.cfg.obs_dim == OBS_DIM
    P0 = model.get_parameters()
    assert P0[first_kernel(model)].shape == (OBS_DIM, 64)
    model.learn(40)
    assert model.num_timesteps == 40 and model.n_updates >= 20 and model.engine.replay_size() == 40
    P1 = model.get_parameters()
    assert all(np.isfinite(v).all() for v in P1.values())
    assert not np.array_equal(P0[first_kernel(model)], P1[first_kernel(model)])
    # predict: one image, a batch of images, uint8 and float32 -- the bins of the pre-flattened rows
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (3,) + SHAPE).astype(np.uint8)
    if normalize:
        imgs_in = env.normalize_obs(imgs.astype(np.float32)).astype(np.float32)
    else:
        imgs_in = imgs
    rows = np.asarray(imgs_in, np.float32).reshape(3, OBS_DIM)
    want = np.asarray([model._bins_to_env_action(b) for b in np.concatenate([model.engine.act_bins(r[None]) for r in rows])])
    one, _ = model.predict(imgs_in[0])
    many, _ = model.predict(imgs_in)
    assert np.shape(one) == np.shape(want[0]) and np.array_equal(one, want[0])
    assert many.shape[0] == 3 and np.array_equal(many, want)
    assert np.array_equal(model.predict(np.asarray(imgs_in, np.float32))[0], many)
    # save / load: parameters equal, the observation space back with its shape
    path = str(tmp_path / "model")
    model.save(path)
    loaded = type(model).load(path)
    assert tuple(loaded.observation_space.shape) == SHAPE
    P2 = loaded.get_parameters()
    assert P2[first_kernel(model)].shape == (OBS_DIM, 64)
    assert set(P2) == set(P1) and all(np.array_equal(P1[k], P2[k]) for k in P1)
    assert np.array_equal(loaded.predict(imgs_in)[0], many)
    # a subset of the parameters
    k = first_kernel(model)
    loaded.load_parameters({k: np.zeros_like(P1[k])}, exact_match=False)
    P3 = loaded.get_parameters()
    assert not P3[k].any() and all(np.array_equal(P1[n], P3[n]) for n in P1 if n != k)
    with pytest.raises(RuntimeError):
        loaded.load_parameters({"deepq/model/conv/weights:0": np.zeros(3, np.float32)}, exact_match=False)
    loaded.set_env(make_env(algo, normalize, seed=3))
    loaded.learn(16)
    for m in (model, loaded):
        m.engine.close()


def test_cnn_policy_still_raises():
    with pytest.raises(NotImplementedError):
        DQN(CnnPolicy, make_env("dqn", False))
    with pytest.raises(NotImplementedError):
        DQN(CnnPolicy, make_env("dqn", False), policy_kwargs={"layer_norm": True})


def test_layer_normalised_policy_takes_the_image():
    model = DQN(LnMlpPolicy, make_env("dqn", False), batch_size=8, learning_starts=8, buffer_size=32, seed=0)
    assert model.get_parameters()["deepq/model/action_value/LayerNorm/gamma:0"].shape == (64,)
    model.learn(20)
    assert model.n_updates >= 10 and all(np.isfinite(v).all() for v in model.get_parameters().values())
    model.engine.close()


def test_image_is_flattened_in_c_order_and_not_divided_by_255():
    """Against the float64 restatement of tests/q_layer_norm_util.py (layer norm off) on the model's own parameters: the Q-values
    of a raw 0 ... 255 image are those of its C-order flattening fed as it is, and ONE non-zero pixel at (i, j, c) moves exactly
    the contribution of kernel row (i * 64 + j) * 2 + c -- neither the F-order row nor the value / 255 would pass."""
    model = make_model("dqn", make_env("dqn", False))
    rng = np.random.default_rng(1)
    P = model.get_parameters()
    for k in P:                                              # biases away from zero: everything takes part
        if k.endswith("biases:0"):
            P[k] = rng.uniform(-0.1, 0.1, P[k].shape).astype(np.float32)
    model.load_parameters(P)
    spec = od.QSpec(algo="dqn", obs_dim=OBS_DIM, n_branches=1, n_bins=6)
    ref = ql.QRef64(spec, model.get_parameters(), layer_norm=False)
    q_of = lambda img: model.engine.q_values(np.asarray(img, np.float32)[None])
    tol = lambda r: 2e-5 + 2e-4 * np.abs(r)                  # the forward tolerance of q_parity_util.run_and_compare
    img = rng.integers(0, 256, SHAPE).astype(np.uint8)
    want = ref.q_values(img.astype(np.float64).reshape(1, OBS_DIM))
    got = q_of(img)
    assert (np.abs(got - want) <= tol(want)).all(), np.abs(got - want).max()
    scaled = ref.q_values(img.astype(np.float64).reshape(1, OBS_DIM) / 255.0)
    assert (np.abs(got - scaled) > 100 * tol(scaled)).any()                      # (the test tells the two apart)
    i, j, c = 37, 5, 1
    one = np.zeros(SHAPE, np.float32)
    one[i, j, c] = 200.0
    flat_c, flat_f = np.zeros((1, OBS_DIM)), np.zeros((1, OBS_DIM))
    flat_c[0, (i * 64 + j) * 2 + c] = 200.0
    flat_f[0, np.ravel_multi_index((i, j, c), SHAPE, order="F")] = 200.0
    want, other, got = ref.q_values(flat_c), ref.q_values(flat_f), q_of(one)
    assert (np.abs(got - want) <= tol(want)).all(), np.abs(got - want).max()
    assert (np.abs(want - other) > 100 * tol(want)).any()
    # ... and through predict: the greedy action of the image is the arg-max of the reference
    top = np.sort(ref.q_values(img.astype(np.float64).reshape(1, OBS_DIM)), axis=2)[0, 0, -2:]
    assert top[1] - top[0] > 1e-4
    assert int(model.predict(img)[0]) == int(ref.q_values(img.astype(np.float64).reshape(1, OBS_DIM)).argmax(axis=2)[0, 0])
    model.engine.close()


@pytest.mark.parametrize("algo,n", [("dqn", 1), ("bdq", 2)])
def test_learn_with_device_statistics_equals_host_statistics_on_images(algo, n):
    """tests/q_device_norm_learn_util.py's comparison on the image env: statistics of the image's shape on the device
    (norm_update_kernel over 8192 elements, observe-once, replay_add_observed) == the host path, bit for bit."""
    def run(device_norm):
        env = make_env(algo, True, n=n)
        model = make_model(algo, env, device_norm=device_norm, batch_size=8, learning_starts=10, buffer_size=32)
        spy = dl.Spy(model)
        model.learn(36)
        out = dl.result(model, env)
        assert env.obs_rms.mean.shape == SHAPE
        model.engine.close()
        return out, spy
    host, spy_h = run(False)
    dev, spy_d = run(True)
    dl.assert_same(host, dev, "%s n=%d" % (algo, n))
    assert spy_h.count("replay_add") == 36 // n and not spy_h.count("observe")
    assert spy_d.count("replay_add") == 0 and spy_d.count("replay_add_observed") == 36 // n and spy_d.count("set_obs_stats") == 1


def test_checkpoint_of_an_image_model_continues(tmp_path, monkeypatch):
    monkeypatch.setenv("GRL_CHECKPOINT_STATE", "1")
    env = make_env("dqn", True)
    model = make_model("dqn", env)
    model.learn(24)
    path = str(tmp_path / "ck")
    model.save(path)
    loaded = DQN.load(path, env=make_env("dqn", True, seed=1))
    assert loaded.num_timesteps == 24 and loaded.engine.replay_size() == 24
    P, Q = model.get_parameters(), loaded.get_parameters()
    assert all(np.array_equal(P[k], Q[k]) for k in P)
    loaded.learn(12, reset_num_timesteps=False)
    assert loaded.num_timesteps == 36
    for m in (model, loaded):
        m.engine.close()
