"""Shared body of the DQN / BDQ learn-loop checks with the VecNormalize statistics on the device (``device_norm=True``) against
the host path (``device_norm=False``): tests/test_q_device_norm_learn_host.py runs it on the emulation build, tests/
test_gpu_q_device_norm_learn.py on the MI355X.  Both runs see the same environments (grasp_rl.synthetic.ReachGraspEnv, seed 0)
and must agree bit for bit in everything the loop leaves behind."""
import pickle

import numpy as np

from grasp_rl.sb.dqn import BDQ, DQN
from grasp_rl.sb.vec_env import DummyVecEnv, VecNormalize
from grasp_rl.synthetic import ReachGraspEnv

TOTAL, HALF = 300, 150            # HALF: 10 episodes of 15 steps of one environment -- the checkpoint falls where an episode starts
CASES = [(algo, per, n) for algo in ("dqn", "bdq") for per in (False, True) for n in (1, 16)]


class RecordingReach(ReachGraspEnv):
    """Remembers the generator state in front of its latest reset: an environment built later continues from there."""

    def reset(self):
        self.before_reset = self._rng.bit_generator.state
        return super().reset()


def make_env(algo, n, resume_from=None):
    action = "discrete" if algo == "dqn" else "box"
    envs = [RecordingReach("vector", seed=s, action=action, n_discrete=5) for s in range(n)]
    if resume_from is not None:       # the generators stand where the saved run's last auto-reset found them
        for e, old in zip(envs, resume_from.venv.envs):
            e._rng.bit_generator.state = old.before_reset
    return VecNormalize(DummyVecEnv([(lambda e=e: e) for e in envs]), norm_obs=True, norm_reward=True, clip_obs=10.0)


def make_model(algo, env, per, device_norm, total=TOTAL):
    kw = dict(batch_size=32, learning_starts=50, buffer_size=256, seed=0, prioritized_replay=per, device_norm=device_norm,
              prioritized_replay_beta_iters=TOTAL, exploration_fraction=0.25 * TOTAL / total, exploration_final_eps=0.05,
              target_network_update_freq=40)
    if algo == "dqn":
        return DQN("MlpPolicy", env, policy_kwargs={"layers": [64, 64]}, learning_rate=1e-3, **kw)
    return BDQ("MlpActPolicy", env, policy_kwargs={"layers": [[64, 64], [32], [32]]}, num_actions_pad=33, **kw)


class Spy:
    """Counts the engine calls the device path exists to remove, with the loop's counter at the time of the call."""

    def __init__(self, model):
        self.calls = []
        eng = model.engine
        for name in ("set_obs_stats", "replay_add", "replay_add_observed", "observe"):
            real = getattr(eng, name)
            setattr(eng, name, (lambda *a, _r=real, _n=name, **k: (self.calls.append((_n, model.num_timesteps)), _r(*a, **k))[1]))

    def count(self, name, after=-1):
        return sum(1 for n, t in self.calls if n == name and t > after)


def result(model, env):
    eng = model.engine
    eng.synchronize()
    out = {"vecnormalize": pickle.dumps(env), "counters": (model.num_timesteps, model.n_updates),
           "rng": repr(model._rng.bit_generator.state), "replay_size": eng.replay_size()}
    for k, v in model.get_parameters().items():
        out["p:" + k] = np.asarray(v, np.float32).reshape(-1).view(np.uint32).copy()
    flat = np.ascontiguousarray(eng.be.to_host(eng.replay)).view(np.uint32)
    for k, seg in enumerate(eng.replay_segments()):
        lo, hi = eng._segment_span(seg, eng.replay_size())
        out["replay:%d" % k] = flat[lo:hi].copy()
    return out


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        same = np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]
        assert same, "%s: %s differs" % (what, k)


def run(algo, per, n, device_norm):
    env = make_env(algo, n)
    model = make_model(algo, env, per, device_norm)
    spy = Spy(model)
    model.learn(TOTAL)
    out = result(model, env)
    model.engine.close()
    return out, spy, model


def check_device_equals_host(algo, per, n):
    host, spy_h, _ = run(algo, per, n, False)
    dev, spy_d, model = run(algo, per, n, True)
    steps = -(-TOTAL // n) * n
    assert host["counters"][0] == steps and host["counters"][1] > (TOTAL - 50) // 2 and host["replay_size"] == 256
    assert_same(host, dev, "%s per=%s n=%d" % (algo, per, n))
    # host path: one replay_add per vectorised step and one push per step that updates; device path: neither after the first step
    assert spy_h.count("replay_add") == steps // n and spy_h.count("set_obs_stats", after=50) > 0 and not spy_h.count("observe")
    assert spy_d.count("replay_add") == 0 and spy_d.count("set_obs_stats", after=0) == 0
    assert spy_d.count("set_obs_stats") == 1                                   # the upload when the wrapper is attached
    assert spy_d.count("replay_add_observed") == steps // n and spy_d.count("observe") == steps // n + 1
    assert model._vec_normalize_env._dev is None                               # detached when learn returned


def check_checkpoint_continues(algo, per, tmp_path, monkeypatch):
    """learn(HALF) -> save with GRL_CHECKPOINT_STATE=1 -> load into a new model -> learn(TOTAL - HALF) == learn(TOTAL), with the
    statistics on the device throughout."""
    whole, _, _ = run(algo, per, 1, True)
    monkeypatch.setenv("GRL_CHECKPOINT_STATE", "1")
    env = make_env(algo, 1)
    model = make_model(algo, env, per, True, total=HALF)
    model.learn(HALF)
    path = str(tmp_path / "model")
    model.save(path)
    model.engine.close()
    env2 = make_env(algo, 1, resume_from=env)
    model2 = type(model).load(path, env=env2, device_norm=True)
    assert model2.num_timesteps == HALF
    spy = Spy(model2)
    model2.learn(TOTAL - HALF, reset_num_timesteps=False)
    assert spy.count("set_obs_stats") == 0 and spy.count("replay_add") == 0     # restored: the device holds the statistics already
    out = result(model2, env2)
    model2.engine.close()
    assert_same(whole, out, "%s per=%s resumed at %d" % (algo, per, HALF))
