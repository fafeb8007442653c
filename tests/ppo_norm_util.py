"""Shared bodies of the "VecNormalize observation statistics on PPO2 / TRPO handles" checks: run on the emulation build by
tests/test_hostemu_ppo_norm.py and tests/test_ppo_norm_learn_host.py, on the MI355X by tests/test_gpu_ppo_norm.py and
tests/test_gpu_ppo_norm_learn.py.  `make(kind, obs_dim, n_envs, normalize, n_steps=...)` builds a PpoEngine ("ppo") or a TrpoEngine
("trpo") with towers [64, 64]; `read_err()` returns what the library wrote to stderr since the last call (GRL_PLAN_DUMP is set by
the caller).

Every comparison is exact -- raw words where floats are compared, a NaN mask only where a NaN was put in on purpose.  Exactness is
derived, not measured: device and host perform the same IEEE operations in the same order (sequential float32 sums with
contraction off for the batch moments, `batch_var * n` as a float32 product, then float64 + - x / sqrt for the Chan merge, the
standard deviation and the normalised value, rounded to float32 once), which is the project's standard for the SAC and DQN / BDQ
device paths (tests/q_device_norm_util.py).  The epsilon under the root is the wrapper's Python float on both sides
(grl_ppo_config.norm_eps64).

Shapes (the smallest at which each decision can go wrong): observation widths 1, 3 (row padding to 4, which must read zero), 255,
256, 257 (both sides of a workgroup of ppo_observe_kernel), 2048, 2049 (both sides of the one-launch act; the route is asserted
from the plan dump); rows 1 (batch variance exactly 0), 2, 16, 17.  Inputs: column 0 constant; one row per call with +1e4 in the
odd and -1e4 in the even columns, so that the clip is hit on both signs once the loaded statistics (count 1e6) are in place; call
2 starts from statistics loaded with grl_set_running_stats; call 3 goes without GRL_OBSERVE_UPDATE_STATS and carries a NaN."""
import os
import pickle

import numpy as np

import ppo_util as pu
import trpo_util as tu
from grasp_rl import _capi
from grasp_rl.sb.running_mean_std import RunningMeanStd
from q_device_norm_util import host_normalize, words

ERR_INVALID, ERR_STATE = -1, -3
WIDTHS = (1, 3, 255, 256, 257, 2048, 2049)
ROWS = (1, 2, 16, 17)
TRPO_WIDTHS = (3, 257)
N_CALLS = 5
A = 2
TOWER = (64, 64)
CLIP, EPS = 10.0, 1e-8
OBSERVE_CASES = [("ppo", w, n) for w in WIDTHS for n in ROWS] + [("trpo", w, 1) for w in TRPO_WIDTHS]


def engine_config(kind, obs_dim, n_envs, normalize, n_steps=N_CALLS, nmb=1):
    """(GrlConfig, second block) of the handles these checks build; normalize 0 or 2 (or what a refusal test asks for)."""
    norm = dict(normalize=normalize, clip_obs=CLIP, norm_eps=EPS) if normalize else {}
    if kind == "ppo":
        return _capi.make_ppo_config(obs_dim, A, n_envs=n_envs, n_steps=n_steps, nminibatches=nmb, pi_layers=TOWER, vf_layers=TOWER, **norm)
    assert n_envs == 1
    return _capi.make_trpo_config(obs_dim, A, timesteps_per_batch=n_steps, pi_layers=TOWER, vf_layers=TOWER, **norm)


def init_params(obs_dim):
    return pu.init_params(obs_dim, A, TOWER, TOWER, seed=3)


def raw_rows(rng, n, obs_dim):
    x = (rng.normal(0.5, 2.0, (n, obs_dim)) * (1.0 + np.arange(obs_dim) % 3)).astype(np.float32)
    x[:, 0] = 3.25
    x[n // 2, 1::2] += np.float32(1e4)
    x[n // 2, 2::2] -= np.float32(1e4)
    return x


def same(got, want, what, nan=False):
    """Raw words; nan: the NaNs sit where the expected ones do, every other element by its words."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if nan:
        hole = np.isnan(want)
        assert np.array_equal(np.isnan(got), hole), what
        got, want = np.where(hole, 0, got).astype(want.dtype), np.where(hole, 0, want).astype(want.dtype)
    else:
        assert not np.isnan(want).any(), what
    assert np.array_equal(words(got), words(want)), what


def same_stats(eng, ref, what):
    m, v, c = eng.get_obs_stats(ref.mean.shape)
    assert m.dtype == np.float64 and v.dtype == np.float64
    same(m, np.asarray(ref.mean, np.float64), what + ": mean")
    same(v, np.asarray(ref.var, np.float64), what + ": var")
    assert np.float64(c).tobytes() == np.float64(ref.count).tobytes(), what + ": count"


# ------------------------------------------------------------------------------------------------------------ 1. kernel and ABI
def check_observe(make, read_err, kind, obs_dim, n):
    """Five successive grl_observe calls against RunningMeanStd.update and VecNormalize.normalize_obs(...).astype(float32): the
    statistics after every call, "ppo_obs_n", the slot of "ppo_obs" that grl_ppo_step(NULL) fills, and what that step returns
    against a normalize = 0 handle handed the host's rows; then grl_ppo_finish(NULL) against that handle's finish."""
    read_err()
    eng = make(kind, obs_dim, n, 2)
    route = pu.route_from_dump(read_err())
    assert ("one" in route) == (obs_dim <= 2048) and ("list_obs" in route) == (obs_dim > 2048), route
    twin = make(kind, obs_dim, n, 0)
    try:
        ldo = eng.ldo
        assert ldo == (obs_dim + 3) // 4 * 4
        ref = RunningMeanStd(shape=(obs_dim,))
        same_stats(eng, ref, "a new handle")                         # RunningMeanStd(): mean 0, var 1, count 1e-4
        rng = np.random.default_rng(100 * obs_dim + n)
        clipped = set()
        for k in range(N_CALLS):
            x = raw_rows(rng, n, obs_dim)
            update, nan = k != 3, k == 3
            if k == 2:                                               # the starting point is taken as given
                ref.mean, ref.var, ref.count = ref.mean * 0.5 + 0.25, np.full(obs_dim, 0.5), 1e6
                eng.set_running_stats(ref.mean, ref.var, ref.count)
                same_stats(eng, ref, "loaded")
            if nan:
                x[n - 1, obs_dim // 2] = np.nan
            else:
                ref.update(x)
            eng.observe(x, update_stats=update)
            same_stats(eng, ref, "call %d" % k)                      # (call 3: unchanged)
            want = host_normalize(np.asarray(ref.mean, np.float64), np.asarray(ref.var, np.float64), x, CLIP, EPS)
            assert want.dtype == np.float32 and want.shape == (n, obs_dim) and np.isnan(want).sum() == (1 if nan else 0)
            clipped |= set(np.unique(want[np.abs(want) == CLIP]).tolist())
            rows = eng.fetch("ppo_obs_n", (n, ldo))
            same(rows[:, :obs_dim], want, "ppo_obs_n, call %d" % k, nan)
            assert not words(rows[:, obs_dim:]).any(), "padding of ppo_obs_n"
            done, eps = (rng.random(n) < 0.3).astype(np.float32), rng.normal(0.0, 1.0, (n, A)).astype(np.float32)
            out, out_t = eng.step(None, done, eps), twin.step(want, done, eps)
            slot = eng.fetch("ppo_obs", (n, N_CALLS, ldo))[:, k]
            same(slot[:, :obs_dim], want, "ppo_obs slot %d" % k, nan)
            assert not words(slot[:, obs_dim:]).any(), "padding of ppo_obs"
            for name, a, b in zip(("action", "value", "neglogp"), out, out_t):
                same(a, b, "%s of step %d" % (name, k), nan)
            rew = rng.normal(0.0, 1.0, n).astype(np.float32)
            eng.rewards(rew)
            twin.rewards(rew)
        if obs_dim >= 3:
            assert clipped == {-CLIP, CLIP}, clipped                 # the clip was hit on both signs
        assert x[:, 0].min() == x[:, 0].max() == np.float32(3.25)
        last_done = (rng.random(n) < 0.3).astype(np.float32)
        eng.finish(None, last_done)                                  # the rows of the last observe
        twin.finish(want, last_done)
        for name, shape in (("ppo_last_v", (n,)), ("ppo_adv", (n, N_CALLS)), ("ppo_ret", (n, N_CALLS)), ("ppo_old_v", (n, N_CALLS))):
            same(eng.fetch(name, shape), twin.fetch(name, shape), name, nan=True)
        same(eng.fetch("ppo_obs", (n, N_CALLS, ldo)), twin.fetch("ppo_obs", (n, N_CALLS, ldo)), "rollout observations", nan=True)
    finally:
        eng.close()
        twin.close()


def check_refusals(make, lib):
    """normalize 1 and 3 by name; grl_observe with n != n_envs; grl_ppo_step / _finish(NULL) with nothing observed and on a
    normalize = 0 handle; grl_norm_update and grl_replay_add_observed on the handle; every statistics call on a normalize = 0 one."""
    import ctypes as C
    err = lambda: lib.grl_last_error().decode()
    s = _capi.GrlSizes()
    for mode in (1, 3):
        cfg, ppo = engine_config("ppo", 5, 2, mode)
        assert cfg.normalize == mode
        assert lib.grl_ppo_query_sizes(C.byref(cfg), C.byref(ppo), C.byref(s)) == ERR_INVALID
        assert "normalize %d" % mode in err() and "rewards" in err(), err()
        cfg, trpo = engine_config("trpo", 5, 1, mode)
        assert lib.grl_trpo_query_sizes(C.byref(cfg), C.byref(trpo), C.byref(s)) == ERR_INVALID
        assert "normalize %d" % mode in err() and "rewards" in err(), err()
    z = np.zeros((4, 5), np.float32)
    d = np.zeros(4, np.float32)
    o = np.zeros(16, np.float32)
    p, dp, op = z.ctypes.data, d.ctypes.data, o.ctypes.data
    m64 = np.zeros(5, np.float64)
    cnt = C.c_double()
    for kind, n in (("ppo", 2), ("trpo", 1)):
        eng = make(kind, 5, n, 2)
        h = eng.h
        for bad in (n + 1, n - 1) if n > 1 else (n + 1,):
            assert lib.grl_observe(h, p, bad, 1) == ERR_INVALID and "n_envs" in err(), err()
        assert lib.grl_observe(h, p, n, 2) == ERR_INVALID
        assert lib.grl_ppo_step(h, None, dp, None, op, op, op) == ERR_STATE and "grl_observe" in err(), err()
        for _ in range(eng.n_steps):                                 # (a full rollout through the host path, so that finish can be asked)
            eng.step(z[:n], d[:n])
            eng.rewards(d[:n])
        assert lib.grl_ppo_finish(h, None, dp) == ERR_STATE and "grl_observe" in err(), err()
        assert lib.grl_norm_update(h, p, n) == ERR_STATE
        assert lib.grl_replay_add_observed(h, p, p, p, n, None, None, 0) == ERR_STATE
        eng.observe(z[:n], update_stats=True)
        eng.finish(None, d[:n])
        eng.close()
        eng = make(kind, 5, n, 0)
        h = eng.h
        word = ("PPO" if kind == "ppo" else "TRPO") + " handle"
        assert lib.grl_ppo_step(h, None, dp, None, op, op, op) == ERR_STATE and "normalize = 0" in err(), err()
        for call in (lambda: lib.grl_observe(h, p, n, 1), lambda: lib.grl_norm_update(h, p, n),
                     lambda: lib.grl_set_obs_stats(h, m64.ctypes.data, m64.ctypes.data, 1.0),
                     lambda: lib.grl_set_running_stats(h, m64.ctypes.data, m64.ctypes.data, 1.0),
                     lambda: lib.grl_get_obs_stats(h, m64.ctypes.data, m64.ctypes.data, C.byref(cnt)),
                     lambda: lib.grl_replay_add_observed(h, p, p, p, n, None, None, 0)):
            assert call() == ERR_STATE and word in err(), err()
        eng.close()


# ------------------------------------------------------------------------------------------------------------ 2. unchanged ground
PARENT_CASES = (("ppo", "odd_towers"), ("ppo", "wide_obs"), ("trpo", "odd"))


def parent_snapshot_text(make_case_engine, read_err):
    """`== kind name`, the six numbers grl_*_query_sizes returns and the GRL_PLAN_DUMP text of a normalize = 0 handle of each of
    PARENT_CASES (tests/ppo_util.py, tests/trpo_util.py); make_case_engine(module, case) builds the handle.  The text of
    tests/golden/ppo_plan_dump_parent.txt was written by this function on the parent commit's emulation build."""
    out = []
    for kind, name in PARENT_CASES:
        mod = pu if kind == "ppo" else tu
        read_err()
        eng = make_case_engine(mod, mod.make_case(name))
        assert eng.cfg.normalize == 0
        s = eng.sizes
        sizes = "sizes %d %d %d %d %d %d" % (s.state_bytes, s.grads_bytes, s.work_bytes, s.replay_bytes, s.n_params, s.n_trainable)
        eng.close()
        out.append("== %s %s\n%s\n%s" % (kind, name, sizes, read_err()))
    return "".join(out)


def check_plan_is_the_parents(make_case_engine, read_err):
    want = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_plan_dump_parent.txt")).read()
    assert want.count("== ") == len(PARENT_CASES) and "grl plan: trpo vec" in want and "ppo_act       launch list" in want
    got = parent_snapshot_text(make_case_engine, read_err)
    assert got == want


def check_host_path_unchanged(make, kind, obs_dim=13, n=3, T=7):
    """A normalize = 2 handle driven down the host path (rows uploaded, no observe) leaves the parameters, the Adam moments and
    the rollout of a normalize = 0 handle."""
    n = n if kind == "ppo" else 1
    rng = np.random.default_rng(17)
    obs = rng.normal(0.0, 1.0, (T + 1, n, obs_dim)).astype(np.float32)
    eps = rng.normal(0.0, 1.0, (T, n, A)).astype(np.float32)
    done = (rng.random((T + 1, n)) < 0.2).astype(np.float32)
    rew = rng.normal(0.0, 1.0, (T, n)).astype(np.float32)
    perm = np.stack([np.random.RandomState(e).permutation(n * T) for e in range(2)]).astype(np.int32)
    outs = []
    for normalize in (0, 2):
        eng = make(kind, obs_dim, n, normalize, n_steps=T)
        for t in range(T):
            eng.step(obs[t], done[t], eps[t])
            eng.rewards(rew[t])
        eng.finish(obs[T], done[T])
        roll = {name: eng.fetch(name).copy() for name in ("ppo_obs", "ppo_act", "ppo_old_v", "ppo_old_nlp", "ppo_adv", "ppo_ret")}
        eng.train(perm) if kind == "ppo" else eng.update(None)
        roll.update(("p:" + k, np.asarray(v, np.float32)) for k, v in eng.get_parameters().items())
        roll["adam_m"], roll["adam_v"] = eng.fetch("adam_m").copy(), eng.fetch("adam_v").copy()
        outs.append(roll)
        eng.close()
    assert set(outs[0]) == set(outs[1])
    moved = False
    for k in outs[0]:
        same(outs[1][k], outs[0][k], k)
        moved = moved or (k.startswith("p:") and not np.array_equal(outs[0][k], init_params(obs_dim).get(k[2:])))
    assert moved or kind == "trpo"      # (a TRPO line search may restore the parameters; the PPO2 update always moves them)


# ------------------------------------------------------------------------------------------------------------ 3. model level
LEARN_CASES = [("ppo2", 1), ("ppo2", 4), ("trpo", 1)]
# PPO2: n_steps 8, minibatches of 16 rows, two rollouts.  One environment has 8 rows per rollout, so its n_steps is 16 (one
# minibatch of 16).  TRPO: timesteps_per_batch 128, the smallest at which the value fit (minibatches of 128 rows) runs at all --
# without it there are no Adam moments to compare.
ROLLOUTS = 2


def make_env(n, kind="vector"):
    from grasp_rl.sb.monitor import Monitor
    from grasp_rl.sb.vec_env import DummyVecEnv, VecNormalize
    from grasp_rl.synthetic import ReachGraspEnv
    envs = [Monitor(ReachGraspEnv(kind, seed=s)) for s in range(n)]
    return VecNormalize(DummyVecEnv([(lambda e=e: e) for e in envs]), norm_obs=True, norm_reward=True, clip_obs=10.0)


def model_args(algo, n):
    if algo == "ppo2":
        n_steps = 8 if n * 8 >= 16 else 16
        return dict(n_steps=n_steps, nminibatches=n * n_steps // 16, noptepochs=2, seed=0, learning_rate=1e-3,
                    policy_kwargs={"net_arch": [dict(vf=[64, 64], pi=[64, 64])]}), ROLLOUTS * n * n_steps
    return dict(timesteps_per_batch=128, vf_iters=2, seed=0, policy_kwargs={"net_arch": [dict(vf=[64, 64], pi=[64, 64])]}), ROLLOUTS * 128


def make_model(algo, env, device_norm="unset", **over):
    from grasp_rl.sb.ppo2 import PPO2
    from grasp_rl.sb.trpo import TRPO
    kw, total = model_args(algo, env.num_envs)
    kw.update(over)
    if device_norm != "unset":
        kw["device_norm"] = device_norm
    return (PPO2 if algo == "ppo2" else TRPO)("MlpPolicy", env, **kw), total


class Spy:
    """The engine and wrapper calls the device path exists to change: every `observe`, whether `step` / `finish` were handed an
    array, every `attach_device` and wrapper `reset`."""

    def __init__(self, model):
        self.observes, self.arrays, self.nones, self.attached, self.resets = 0, 0, 0, 0, 0
        eng, vn = model.engine, model.get_vec_normalize_env()
        real_observe, real_step, real_finish = eng.observe, eng.step, eng.finish
        real_attach, real_reset = vn.attach_device, vn.reset

        def observe(*a, **k):
            self.observes += 1
            return real_observe(*a, **k)

        def count(obs):
            if obs is None:
                self.nones += 1
            else:
                self.arrays += 1

        def step(obs, *a, **k):
            count(obs)
            return real_step(obs, *a, **k)

        def finish(obs, *a, **k):
            count(obs)
            return real_finish(obs, *a, **k)

        def attach(*a, **k):
            self.attached += 1
            return real_attach(*a, **k)

        def reset(*a, **k):
            self.resets += 1
            return real_reset(*a, **k)

        eng.observe, eng.step, eng.finish, vn.attach_device, vn.reset = observe, step, finish, attach, reset
        self.vn = vn

    def release(self):
        """The wrapper as it was (it is pickled afterwards)."""
        del self.vn.attach_device, self.vn.reset


def result(model, env):
    eng = model.engine
    eng.synchronize()
    assert env._dev is None                                          # detached when learn returned
    out = {"vecnormalize": pickle.dumps(env), "num_timesteps": model.num_timesteps,
           "episodes": [(e["r"], e["l"]) for e in model.ep_info_buf],
           "obs_rms": (words(np.asarray(env.obs_rms.mean, np.float64)).copy(), words(np.asarray(env.obs_rms.var, np.float64)).copy(),
                       np.float64(env.obs_rms.count).tobytes()),
           "ret_rms": (np.float64(env.ret_rms.mean).tobytes(), np.float64(env.ret_rms.var).tobytes(), np.float64(env.ret_rms.count).tobytes())}
    for k, v in model.get_parameters().items():
        out["p:" + k] = words(np.asarray(v, np.float32).reshape(-1)).copy()
    out["adam_m"], out["adam_v"] = words(eng.fetch("adam_m")).copy(), words(eng.fetch("adam_v")).copy()
    return out


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            ok = np.array_equal(a[k], b[k])
        elif isinstance(a[k], tuple) and isinstance(a[k][0], np.ndarray):
            ok = all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a[k], b[k]))
        else:
            ok = a[k] == b[k]
        assert ok, "%s: %s differs" % (what, k)


def run(algo, n, device_norm, callback=None, **over):
    env = make_env(n)
    model, total = make_model(algo, env, device_norm, **over)
    spy = Spy(model)
    model.learn(total, callback=callback)
    spy.release()
    out = result(model, env)
    steps = total // n
    model.engine.close()
    return out, spy, steps


def check_device_equals_host(algo, n):
    host, spy_h, steps = run(algo, n, False)
    dev, spy_d, _ = run(algo, n, True)
    assert host["num_timesteps"] == steps * n and len(host["episodes"]) >= (steps // 15) * n > 0
    assert host["adam_v"].any() and np.frombuffer(host["obs_rms"][2], np.float64)[0] > steps * n
    assert_same(host, dev, "%s n=%d" % (algo, n))
    # host path: no observe, an array per step and finish; device path: one observe per env step and per reset, and no array
    assert spy_h.observes == 0 and spy_h.attached == 0 and spy_h.nones == 0 and spy_h.arrays == steps + ROLLOUTS
    assert spy_d.attached == 1 and spy_d.arrays == 0 and spy_d.nones == steps + ROLLOUTS
    assert spy_d.observes == steps + spy_d.resets and spy_d.resets == (1 if algo == "ppo2" else spy_h.resets)
    if algo == "ppo2":
        assert spy_h.resets == 1


def reading_callback():
    """A user callback that may read new_obs (it declares nothing): 'auto' keeps the host path for it."""
    from grasp_rl.sb.callbacks import BaseCallback

    class Reads(BaseCallback):
        seen = 0

        def _on_step(self):
            obs = self.locals.get("new_obs", self.locals.get("obs"))
            Reads.seen += int(obs is not None)
            return True
    return Reads()


def freezing_callback(at):
    """Clears `training` of the wrapper after `at` calls: the statistics stop moving and the loop goes back to the host."""
    from grasp_rl.sb.callbacks import BaseCallback

    class Freezes(BaseCallback):
        reads_observations = False

        def __init__(self):
            super().__init__()
            self.calls = 0

        def _on_step(self):
            self.calls += 1
            if self.calls == at:
                self.model.get_vec_normalize_env().training = False
            return True
    return Freezes()


def check_switches(monkeypatch):
    """'auto' with a reading callback: host.  GRL_DEVICE_NORM=1 / auto: device.  Unset: nothing attaches."""
    monkeypatch.delenv("GRL_DEVICE_NORM", raising=False)
    base, spy, steps = run("ppo2", 4, "unset")
    assert spy.attached == 0 and spy.observes == 0 and spy.nones == 0
    out, spy, _ = run("ppo2", 4, "auto", callback=reading_callback())
    assert spy.attached == 0 and spy.observes == 0 and spy.nones == 0
    assert_same(base, out, "auto with a reading callback")
    for value in ("1", "auto"):
        monkeypatch.setenv("GRL_DEVICE_NORM", value)
        out, spy, _ = run("ppo2", 4, "unset")
        assert spy.attached == 1 and spy.observes == steps + 1 and spy.arrays == 0, value
        assert_same(base, out, "GRL_DEVICE_NORM=" + value)
    monkeypatch.setenv("GRL_DEVICE_NORM", "0")
    _, spy, _ = run("ppo2", 4, "unset")
    assert spy.attached == 0 and spy.observes == 0


def check_frozen_mid_run(algo, n, at=5):
    host, spy_h, steps = run(algo, n, False, callback=freezing_callback(at))
    dev, spy_d, _ = run(algo, n, True, callback=freezing_callback(at))
    assert_same(host, dev, "%s n=%d frozen at %d" % (algo, n, at))
    assert spy_d.attached == 1 and 0 < spy_d.observes <= at + 1       # the reset and the steps before the callback cleared it
    # the observation in hand when the flag fell was normalised on the device; every later one went up as an array
    assert spy_d.nones == spy_d.observes and spy_d.arrays == steps + ROLLOUTS - spy_d.nones
    assert np.frombuffer(host["obs_rms"][2], np.float64)[0] < (at + 1) * n + 1


def check_loaded_without_env(tmp_path, monkeypatch, load):
    """A zip loaded without env and given a normalised env later: the handle holds no statistics -> one warning, host path."""
    from grasp_rl.sb import logger
    env = make_env(4)
    model, total = make_model("ppo2", env, False)
    path = str(tmp_path / "model")
    model.save(path)
    model.engine.close()
    host, _, _ = run("ppo2", 4, False)
    warned = []
    monkeypatch.setattr(logger, "warn", lambda *a: warned.append(" ".join(str(x) for x in a)))
    env2 = make_env(4)
    loaded = load(path, device_norm=True)
    assert loaded.engine.cfg.normalize == 0 and loaded.device_norm is True
    loaded.set_env(env2)
    spy = Spy(loaded)
    loaded.learn(total)
    spy.release()
    assert len(warned) == 1 and "device_norm" in warned[0] and "host" in warned[0], warned
    assert spy.attached == 0 and spy.observes == 0 and spy.nones == 0
    assert_same(host, result(loaded, env2), "loaded without env")
    loaded.engine.close()
