"""Model-level checkpoint and resume (grasp_rl/sb/checkpoint.py) on the g++ emulation build: run A is ``learn(2T)``; run B is
``learn(T)`` -> ``save_checkpoint`` -> a NEW Python process -> ``load_checkpoint`` -> ``learn(T, reset_num_timesteps=False)``.
Parameters, the whole state arena, the VecNormalize pickle, ``num_timesteps`` / ``n_updates`` / epsilon and every action taken
after the boundary must be EQUAL (raw words, no tolerance).

The environment is deterministic: episodes of EPISODE steps, observations and rewards a pure function of (env seed, episode
index, step in episode), constructible "at episode k".  T is a multiple of N * EPISODE, so the checkpoint falls where every
sub-environment starts an episode and ``reset()`` returns what the uninterrupted run's auto-reset returned there.

The schedules of the Q models measure themselves against ``total_timesteps``: run A (total 2T) and run B's first call (total T)
get the same epsilon schedule in environment steps through ``exploration_fraction`` (0.25 of 2T = 0.5 of T) and an explicit
``prioritized_replay_beta_iters``; B's second call must keep B's first schedule (that is part of the checkpoint).

This file is also the child process: ``python test_checkpoint_learn_host.py <spec.json>``.  tests/test_gpu_checkpoint_learn.py
runs the same procedure on the real library."""
import json
import os
import pickle
import subprocess
import sys
import zipfile

import numpy as np

EPISODE = 6
T = 48            # N = 1: 8 episodes; N = 4: 12 vectorised steps = 2 episodes each; the 64-row ring wraps before 2T
OBS_DIM, ACT_DIM = 6, 2


def _unit(*key):
    """Deterministic float32 values in [-1, 1): a pure function of the key."""
    return np.random.default_rng([int(k) for k in key])


class EpisodeEnv:
    def __init__(self, seed, start_episode=0):
        from grasp_rl.sb.spaces import Box
        self.observation_space = Box(-4.0, 4.0, shape=(OBS_DIM,), dtype=np.float32)
        self.action_space = Box(-1.0, 1.0, shape=(ACT_DIM,), dtype=np.float32)
        self.seed_, self.episode, self.t = int(seed), int(start_episode) - 1, 0
        self.actions = []

    def _obs(self):
        return (2.0 * _unit(self.seed_, self.episode, self.t, 0).standard_normal(OBS_DIM) + 0.5).astype(np.float32).clip(-4, 4)

    def reset(self):
        self.episode, self.t = self.episode + 1, 0
        return self._obs()

    def step(self, action):
        self.actions.append(np.array(action, np.float32).reshape(-1))
        self.t += 1
        rew = float(_unit(self.seed_, self.episode, self.t, 1).standard_normal()) - 0.1 * float(np.sum(np.square(action)))
        return self._obs(), rew, self.t >= EPISODE, {}


def make_env(n, start_episode=0):
    from grasp_rl.sb.vec_env import DummyVecEnv, VecNormalize
    venv = DummyVecEnv([(lambda i=i: EpisodeEnv(100 + i, start_episode)) for i in range(n)])
    return VecNormalize(venv, norm_obs=True, norm_reward=True, clip_obs=10.0)


def _install_emulation(lib):
    from grasp_rl.engine import QEngine, SacEngine
    from grasp_rl.sb.dqn import BDQ
    from grasp_rl.sb.sac import SAC
    from hostemu_backend import NumpyHostBackend
    SAC._engine_factory = staticmethod(lambda cfg, device: SacEngine(cfg, backend=NumpyHostBackend(), lib_path=lib))
    BDQ._engine_factory = staticmethod(lambda cfg, device: QEngine(cfg, backend=NumpyHostBackend(), lib_path=lib))


def model_class(algo):
    from grasp_rl.sb.dqn import BDQ
    from grasp_rl.sb.sac import SAC
    return SAC if algo == "sac" else BDQ


def new_model(spec, env, total):
    if spec["algo"] == "sac":
        return model_class("sac")("MlpPolicy", env, policy_kwargs={"layers": [16, 16]}, buffer_size=64, batch_size=8,
                                  learning_starts=8, seed=3, device_norm=spec["device_norm"], random_exploration=0.1)
    from grasp_rl.sb.policies import BdqMlpActPolicy as MlpActPolicy
    return model_class("bdq")(MlpActPolicy, env, policy_kwargs={"layers": [[16, 16], [8], [8]]}, num_actions_pad=5,
                              buffer_size=64, batch_size=8, learning_starts=8, target_network_update_freq=10, seed=3,
                              prioritized_replay=True, prioritized_replay_beta_iters=2 * T,
                              exploration_fraction=0.25 * (2 * T) / total, exploration_final_eps=0.05)


def load_kwargs(spec):
    return {"device_norm": spec["device_norm"]} if spec["algo"] == "sac" else {}


def result(model, env, skip):
    """Everything the runs are compared on.  skip: vectorised steps before the boundary (their actions are left out)."""
    eng = model.engine
    eng.synchronize()
    out = {"state": np.asarray(eng.be.to_host(eng.state)).view(np.uint32).copy(),
           "vecnormalize": np.frombuffer(pickle.dumps(env), np.uint8),
           "counters": np.array([model.num_timesteps, model.n_updates], np.int64),
           "eps": np.array([model.exploration.value(model.num_timesteps) if hasattr(model, "exploration") else 0.0], np.float64),
           "actions": np.stack([np.stack(e.actions[skip:]) for e in env.venv.envs])}
    for k, v in model.get_parameters().items():
        out["p:" + k] = np.asarray(v, np.float32).reshape(-1).view(np.uint32)
    return out


def resume_and_finish(spec):
    """The second half of run B (a fresh process): restore, continue, write the result."""
    if spec["lib"]:
        _install_emulation(spec["lib"])
    n = spec["n"]
    env = make_env(n, start_episode=T // (n * EPISODE))
    cls = model_class(spec["algo"])
    if spec["how"] == "checkpoint":
        model = cls.load_checkpoint(spec["path"], env, **load_kwargs(spec))
    else:                       # the drop-in route: GRL_CHECKPOINT_STATE=1 is in this process's environment
        model = cls.load(spec["path"], env, **load_kwargs(spec))
    assert model.num_timesteps == T
    model.learn(T, reset_num_timesteps=False)
    np.savez(spec["out"], **result(model, env, 0))


def run_a(spec):
    env = make_env(spec["n"])
    model = new_model(spec, env, 2 * T)
    model.learn(2 * T)
    return result(model, env, T // spec["n"])


def run_b(spec, tmp_path, how="checkpoint"):
    env = make_env(spec["n"])
    model = new_model(spec, env, T)
    model.learn(T)
    path = os.path.join(str(tmp_path), "model_" + how)
    environ = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    environ.pop("GRL_CHECKPOINT_STATE", None)
    if how == "checkpoint":
        model.save_checkpoint(path)
    else:
        os.environ["GRL_CHECKPOINT_STATE"] = "1"
        try:
            model.save(path)
        finally:
            del os.environ["GRL_CHECKPOINT_STATE"]
        environ["GRL_CHECKPOINT_STATE"] = "1"
    assert os.path.isfile(path + ".zip") and os.path.isfile(os.path.join(path + ".state", "host.pkl"))
    model.engine.close()
    child = dict(spec, how=how, path=path, out=os.path.join(str(tmp_path), "b_" + how + ".npz"))
    spec_file = os.path.join(str(tmp_path), "spec_" + how + ".json")
    with open(spec_file, "w") as f:
        json.dump(child, f)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), spec_file], env=environ, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(child["out"]) as z:
        return {k: z[k] for k in z.files}


def assert_equal_runs(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), \
            "%s differs in %d of %d words" % (k, int(np.sum(a[k] != b[k])) if a[k].shape == b[k].shape else -1, a[k].size)


CASES = [("sac", 1, False), ("sac", 4, False), ("sac", 1, True), ("sac", 4, True), ("bdq", 1, False), ("bdq", 4, False)]
IDS = ["%s-n%d%s" % (a, n, "-device_norm" if d else "") for a, n, d in CASES]

if __name__ != "__main__":
    import pytest

    @pytest.fixture
    def emulation(hostemu_lib, monkeypatch):
        from grasp_rl.sb.dqn import BDQ
        from grasp_rl.sb.sac import SAC
        monkeypatch.setattr(SAC, "_engine_factory", SAC._engine_factory)      # restored after the test
        monkeypatch.setattr(BDQ, "_engine_factory", BDQ._engine_factory)
        _install_emulation(hostemu_lib)
        return hostemu_lib

    @pytest.fixture(scope="module")
    def uninterrupted():
        return {}

    def _spec(lib, algo, n, device_norm):
        return {"algo": algo, "n": n, "device_norm": device_norm, "lib": lib}

    def _run_a(cache, spec):
        key = (spec["algo"], spec["n"], spec["device_norm"])
        if key not in cache:
            cache[key] = run_a(spec)
        return cache[key]

    @pytest.mark.parametrize("algo,n,device_norm", CASES, ids=IDS)
    def test_checkpointed_run_equals_uninterrupted_run(emulation, uninterrupted, tmp_path, algo, n, device_norm):
        spec = _spec(emulation, algo, n, device_norm)
        a = _run_a(uninterrupted, spec)
        assert a["counters"][0] == 2 * T and a["counters"][1] > 0 and a["actions"].shape[:2] == (n, T // n)
        assert_equal_runs(a, run_b(spec, tmp_path))

    @pytest.mark.parametrize("algo,n,device_norm", [CASES[3], CASES[5]], ids=[IDS[3], IDS[5]])
    def test_plain_save_and_load_with_the_environment_switch(emulation, uninterrupted, tmp_path, algo, n, device_norm):
        spec = _spec(emulation, algo, n, device_norm)
        assert_equal_runs(_run_a(uninterrupted, spec), run_b(spec, tmp_path, how="save"))

    @pytest.mark.parametrize("algo", ["sac", "bdq"])
    def test_save_without_the_switch_writes_the_same_zip_and_nothing_else(emulation, tmp_path, monkeypatch, algo):
        """Against the zip the same model writes through the bare zip writer (what `save` was before the feature)."""
        from grasp_rl.sb import save_util
        monkeypatch.delenv("GRL_CHECKPOINT_STATE", raising=False)
        spec = _spec(emulation, algo, 1, False)
        env = make_env(1)
        model = new_model(spec, env, T)
        model.learn(2 * EPISODE + 4)
        model.save(str(tmp_path / "with"))
        save_util.save_to_zip(str(tmp_path / "bare"), model._data(), model.get_parameters())
        members = []
        for name in ("with", "bare"):
            with zipfile.ZipFile(str(tmp_path / (name + ".zip"))) as z:
                members.append([(i.filename, z.read(i.filename)) for i in z.infolist()])
        assert members[0] == members[1]
        assert sorted(os.listdir(str(tmp_path))) == ["bare.zip", "with.zip"]
        loaded = model_class(algo).load(str(tmp_path / "with"), make_env(1), **load_kwargs(spec))
        assert loaded.num_timesteps == 0 and loaded._resume is None

    def test_load_checkpoint_refuses_what_does_not_fit(emulation, tmp_path):
        from grasp_rl._capi import GrlError
        spec = _spec(emulation, "sac", 1, False)
        model = new_model(spec, make_env(1), T)
        model.learn(2 * EPISODE)
        path = str(tmp_path / "m")
        model.save(path)
        with pytest.raises(GrlError, match="no checkpoint state"):
            model_class("sac").load_checkpoint(path, make_env(1))
        model.save_checkpoint(path, include_replay=False)
        with pytest.raises(GrlError, match="number of envs|act_batch"):
            model_class("sac").load_checkpoint(path, make_env(4))
        again = model_class("sac").load_checkpoint(path, make_env(1))
        assert again.num_timesteps == 2 * EPISODE and again.engine.replay_size() == 0

else:
    with open(sys.argv[1]) as f:
        resume_and_finish(json.load(f))
