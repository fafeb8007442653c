"""Checkpoint and resume of the PPO2 / TRPO handles and models (include/grl.h: grl_ppo_state_*; grasp_rl/engine.py:
PpoEngine.save_state / load_state; grasp_rl/sb/checkpoint.py), shared by the emulation tests (tests/test_hostemu_ppo_checkpoint.py,
tests/test_ppo_checkpoint_learn_host.py) and the tests on the MI355X (tests/test_gpu_ppo_checkpoint.py,
tests/test_gpu_ppo_checkpoint_learn.py).  Every comparison is equality of raw 32-bit words: nothing here changes arithmetic.

Engine level: two handles are fed the same observations, flags, rewards and permutations (`Feed`, a pure function of the call
index) and draw their actions on the device; one of them is exported at some cursor position and imported into a NEW handle.

Model level: the deterministic `EpisodeEnv` of tests/test_checkpoint_learn_host.py -- observations and rewards a pure function of
(env seed, episode index, step in episode), constructible "at episode k" -- with one addition: a `reset()` that follows a
`reset()` with no step in between returns the same episode again.  stable-baselines' TRPO generator calls `env.reset()` after a
`done` although the DummyVecEnv has reset the environment already; without the addition every episode end would advance the
episode index by two and "seven episodes" would not be `start_episode=7`.  PPO2 never resets twice, so nothing changes for it.

The learning rate of every model is ``lambda f: 3e-4 * f`` over the length of the UNINTERRUPTED run: a run whose first ``learn``
is shorter (the "learn returns, then save" case: learn(T) against learn(2 T)) is handed the same schedule in environment steps,
``3e-4 * (1 - (1 - f) * total / full)``, as tests/test_checkpoint_learn_host.py scales its epsilon schedule; its second call must
then keep the first call's schedule length and update index -- a schedule that started over would show.

This file is also the child process: ``python ppo_checkpoint_util.py <spec.json>`` restores in a fresh process and finishes the
run (a process that has opened the GPU never replaces its program; the parent closes its engine before it starts the child)."""
import ctypes
import json
import os
import pickle
import subprocess
import sys

import numpy as np

EPISODE = 6
OBS_DIM, ACT_DIM = 6, 2


# =================================================================================================== engine level
ENGINE_CASES = {
    "ppo": dict(kind="ppo", normalize=0),
    "ppo_norm": dict(kind="ppo", normalize=2),
    "trpo": dict(kind="trpo", normalize=0),
}
ENG_OBS, ENG_A = 5, 2


def engine_config(kind, normalize=0, **over):
    from grasp_rl import _capi
    norm = dict(normalize=2, clip_obs=5.0, norm_eps=1e-8) if normalize else {}
    if kind == "ppo":
        kw = dict(n_envs=3, n_steps=4, nminibatches=2, pi_layers=(16,), vf_layers=(8, 8), seed=11)
        kw.update(norm)
        kw.update(over)
        return _capi.make_ppo_config(ENG_OBS, ENG_A, **kw)
    kw = dict(timesteps_per_batch=8, pi_layers=(16,), vf_layers=(8, 8), vf_batch=4, cg_iters=3, seed=11)
    kw.update(norm)
    kw.update(over)
    return _capi.make_trpo_config(ENG_OBS, ENG_A, **kw)


def make_engine(kind, backend_factory, lib_path, normalize=0, params=True, **over):
    import ppo_util as pu
    from grasp_rl.engine import PpoEngine, TrpoEngine
    cfg, second = engine_config(kind, normalize, **over)
    eng = (PpoEngine if kind == "ppo" else TrpoEngine)(cfg, second, backend=backend_factory(), lib_path=lib_path)
    if params:
        eng.set_parameters(pu.init_params(ENG_OBS, ENG_A, (16,), (8, 8), 3))
    return eng


def words(eng, arena):
    return np.ascontiguousarray(eng.be.to_host(arena)).view(np.uint32)


def f32_words(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def blob_fields(eng, blob):
    """The host fields behind the two configuration blocks: written, closed, finished, n_parity, observed rows."""
    from grasp_rl import _capi
    off = ctypes.sizeof(_capi.GrlStateHeader) + ctypes.sizeof(_capi.GrlConfig) + ctypes.sizeof(getattr(eng, "trpo", eng.ppo))
    return off, [int(v) for v in np.frombuffer(blob, np.int32, 5, off)]


def with_fields(eng, blob, **fields):
    off, vals = blob_fields(eng, blob)
    for k, name in enumerate(("written", "closed", "finished", "n_parity", "ob_n")):
        if name in fields:
            vals[k] = fields[name]
    return blob[:off] + np.array(vals, np.int32).tobytes() + blob[off + 20:]


class Feed:
    """What the environment and the host loop hand a handle, a pure function of the call index."""

    def __init__(self, eng):
        self.n, self.T, self.R, self.trpo = eng.n_envs, eng.n_steps, eng.R, hasattr(eng, "trpo")

    def obs(self, k):
        return np.random.default_rng([7, k, 0]).normal(0.3, 1.5, (self.n, ENG_OBS)).astype(np.float32)

    def done(self, k):
        return (np.random.default_rng([7, k, 1]).random(self.n) < 0.3).astype(np.float32)

    def rew(self, k):
        return np.random.default_rng([7, k, 2]).normal(0.0, 1.0, self.n).astype(np.float32)

    def perm(self, u):
        rng = np.random.default_rng([7, u, 3])
        return np.stack([rng.permutation(self.R) for _ in range(2)]).astype(np.int32)


class Drive:
    """One handle walking along the feed; `out` collects every word it returns."""

    def __init__(self, eng, k=0, u=0):
        self.eng, self.feed, self.k, self.u, self.out = eng, Feed(eng), k, u, []
        self.norm = eng.cfg.normalize == 2

    def _rows(self):
        obs = self.feed.obs(self.k)
        if self.norm:
            self.eng.observe(obs, update_stats=True)
            return None
        return obs

    def step(self, observed=False):
        """observed: act on the rows the handle holds already (normalize = 2)"""
        act, val, nlp = self.eng.step(None if observed else self._rows(), self.feed.done(self.k))
        self.out += [f32_words(act).ravel(), f32_words(val), f32_words(nlp)]

    def close_slot(self):
        self.eng.rewards(self.feed.rew(self.k))
        self.k += 1

    def finish_and_update(self):
        self.eng.finish(self._rows(), self.feed.done(self.k))
        self.out += [f32_words(self.eng.fetch("ppo_adv")), f32_words(self.eng.fetch("ppo_ret"))]
        if self.feed.trpo:
            self.eng.update(self.feed.perm(self.u))
            m = self.eng.metrics()
            self.out.append(f32_words([m[n] for n in self.eng.METRIC_NAMES]))
        else:
            self.eng.train(self.feed.perm(self.u))
            self.out.append(f32_words(self.eng.metrics()).ravel())
        self.u += 1

    def rollout(self, first=0, open_first=False):
        """Slots first .. n_steps - 1 (open_first: slot `first` is written already), finish, update."""
        for t in range(first, self.feed.T):
            if not (open_first and t == first):
                self.step()
            self.close_slot()
        self.finish_and_update()

    def to(self, position):
        """From an empty rollout to one of the three cursor positions of the continuation case."""
        if position == "open":
            self.step(); self.close_slot(); self.step()
        elif position == "closed":
            for _ in range(self.feed.T):
                self.step(); self.close_slot()
        else:
            assert position == "empty"

    def go_on_from(self, position):
        """The rest of the rollout the position stands in, its update, and one more rollout with its update."""
        if position == "empty":
            self.rollout()
        elif position == "open":
            self.rollout(first=1, open_first=True)
        else:
            self.finish_and_update()
        self.rollout()


def transplant(a, b):
    """What a caller of the C ABI does: copies the two arenas that hold training state, then moves the blob."""
    blob = a.export_state()
    b.be.write(b.state, a.be.to_host(a.state))
    b.be.write(b.replay, a.be.to_host(a.replay))
    b.be.synchronize()
    b.import_state(blob)
    return blob


def assert_same_handle(a, b, what=""):
    sa, sb = words(a, a.state), words(b, b.state)
    assert np.array_equal(sa, sb), "%s: state arenas differ in %d words" % (what, int((sa != sb).sum()))
    ra, rb = words(a, a.replay), words(b, b.replay)
    assert np.array_equal(ra, rb), "%s: rollouts differ in %d words" % (what, int((ra != rb).sum()))
    assert a.export_state() == b.export_state(), "%s: handle blobs differ" % what
    pa, pb = a.get_parameters(), b.get_parameters()
    assert all(np.array_equal(f32_words(pa[n]), f32_words(pb[n])) for n in pa), what


def assert_same_outputs(da, db, what=""):
    assert len(da.out) == len(db.out) and len(da.out) > 0, what
    for i, (x, y) in enumerate(zip(da.out, db.out)):
        assert x.shape == y.shape and np.array_equal(x, y), "%s: output %d differs" % (what, i)


def snapshot(eng):
    """Everything a refused import must leave alone, as raw words."""
    return {"state": words(eng, eng.state).copy(), "replay": words(eng, eng.replay).copy(), "blob": eng.export_state(),
            "work": words(eng, eng.work).copy()}


def assert_untouched(eng, snap, what=""):
    now = snapshot(eng)
    for k in snap:
        assert np.array_equal(np.frombuffer(now[k], np.uint8) if isinstance(now[k], bytes) else now[k],
                              np.frombuffer(snap[k], np.uint8) if isinstance(snap[k], bytes) else snap[k]), "%s: %s changed" % (what, k)


def check_continuation(case, position, backend_factory, lib_path):
    kw = ENGINE_CASES[case]
    a = make_engine(backend_factory=backend_factory, lib_path=lib_path, **kw)
    da = Drive(a)
    da.rollout(); da.rollout()
    da.to(position)
    b = make_engine(backend_factory=backend_factory, lib_path=lib_path, params=False, **kw)
    transplant(a, b)
    cursor = {"empty": (0, 0, False), "open": (2, 1, False), "closed": (a.n_steps, a.n_steps, False)}[position]
    assert a.rollout_cursor() == cursor and b.rollout_cursor() == cursor
    assert_same_handle(a, b, "after the import")
    da.out = []
    db = Drive(b, da.k, da.u)
    da.go_on_from(position)
    db.go_on_from(position)
    assert_same_outputs(da, db, "%s / %s" % (case, position))
    assert_same_handle(a, b, "%s / %s at the end" % (case, position))
    a.close(); b.close()


def check_statistics_parity(kind, backend_factory, lib_path):
    """Exported after an ODD number of grl_observe calls: n_parity is 1 and the next step(obs=None) acts on the restored rows."""
    from grasp_rl._capi import GrlError
    a = make_engine(kind, backend_factory, lib_path, normalize=2)
    da = Drive(a)
    da.rollout(); da.rollout()                       # n_steps + 1 observe calls each
    calls = 2 * (a.n_steps + 1)
    a.observe(da.feed.obs(da.k), update_stats=True)
    assert (calls + 1) % 2 == 1
    b = make_engine(kind, backend_factory, lib_path, normalize=2, params=False)
    blob = transplant(a, b)
    _, (written, closed, finished, parity, rows) = blob_fields(a, blob)
    assert (written, closed, finished, parity, rows) == (0, 0, 0, 1, a.n_envs)
    fresh = make_engine(kind, backend_factory, lib_path, normalize=2)
    try:
        fresh.step(None, da.feed.done(da.k))
        raise AssertionError("a handle that never observed acted on rows it does not hold")
    except GrlError as e:
        assert "no grl_observe call" in str(e)
    fresh.close()
    da.out = []
    db = Drive(b, da.k, da.u)
    for d in (da, db):
        d.step(observed=True)
        d.close_slot()
        d.rollout(first=1)
    assert_same_outputs(da, db, "statistics parity")
    assert_same_handle(a, b, "statistics parity")
    a.close(); b.close()


def check_save_and_load(kind, normalize, include_replay, backend_factory, lib_path, path):
    """save_state -> destroy -> a new engine -> load_state, with one slot open; include_replay False restores an empty rollout
    and everything else equal."""
    a = make_engine(kind, backend_factory, lib_path, normalize=normalize)
    da = Drive(a)
    da.rollout()
    da.to("open")
    meta = a.save_state(path, include_replay=include_replay, extra={"host.pkl": b"host"})
    assert sorted(os.listdir(path)) == sorted(["handle.bin", "host.pkl", "meta.json", "state.bin"] + (["replay_0.bin"] if include_replay else []))
    assert meta["include_replay"] == include_replay and meta["segments"] == [[0, 4 * int(a.replay.shape[0]), 0]]
    b = make_engine(kind, backend_factory, lib_path, normalize=normalize, params=False)
    b.load_state(path)
    if include_replay:
        assert b.rollout_cursor() == (2, 1, False)
        assert_same_handle(a, b, "loaded")
        da.out = []
        db = Drive(b, da.k, da.u)
        da.go_on_from("open"); db.go_on_from("open")
        assert_same_outputs(da, db, "after load_state")
        assert_same_handle(a, b, "after load_state, at the end")
    else:
        assert b.rollout_cursor() == (0, 0, False)
        a.reset_rollout()                        # what is left to differ: the cursor (its device mirror is a word of the state arena)
        assert np.array_equal(words(a, a.state), words(b, b.state))
        assert a.export_state() == b.export_state()
        Drive(b, da.k, da.u).rollout()           # ... and the empty rollout is usable
    a.close(); b.close()


def _refusals(eng, blob, other_cfg, other_second, other_kind, second_name):
    """(blob, what the refusal says) for every way grl_ppo_state_import refuses"""
    from grasp_rl import _capi
    C = ctypes
    hsz = C.sizeof(_capi.GrlStateHeader)

    def header(**kw):
        hd = _capi.GrlStateHeader.from_buffer_copy(blob[:hsz])
        for k, v in kw.items():
            setattr(hd, k, v)
        return bytes(hd) + blob[hsz:]

    T, N = eng.n_steps, eng.n_envs
    return [
        (blob[:10], "truncated"),
        (blob[:-4], "truncated"),
        (blob + b"\0\0\0\0", "truncated"),
        (b"XXXX" + blob[4:], "wrong magic"),
        (header(version=_capi.GrlStateHeader.from_buffer_copy(blob[:hsz]).version + 1), "library version"),
        (header(layout=7), "layout version 7"),
        (other_cfg, r"another configuration: grl_config\.gamma differs"),
        (other_second, r"another configuration: %s differs" % second_name),
        (other_kind, "written by a (PPO|TRPO) handle, this is a (PPO|TRPO) handle"),
        (header(config_hash=1), "damaged \\(configuration hash\\)"),
        (with_fields(eng, blob, closed=T + 1, written=T + 1), "damaged \\(host fields out of range\\)"),
        (with_fields(eng, blob, closed=-1, written=0), "damaged \\(host fields out of range\\)"),
        (with_fields(eng, blob, closed=1, written=3), "damaged \\(host fields out of range\\)"),
        (with_fields(eng, blob, closed=2, written=1), "damaged \\(host fields out of range\\)"),
        (with_fields(eng, blob, ob_n=N + 1), "damaged \\(host fields out of range\\)"),
    ]


def check_refusals(kind, backend_factory, lib_path):
    """Every refusal of grl_ppo_state_import is raised by name, is GRL_ERR_INVALID and leaves the handle as it was."""
    import pytest
    from grasp_rl._capi import GrlError

    def engine(k, **over):
        return make_engine(k, backend_factory, lib_path, normalize=2, **over)
    other = "trpo" if kind == "ppo" else "ppo"
    eng = engine(kind)
    d = Drive(eng)
    d.rollout()
    d.to("open")
    blob = eng.export_state()

    def blob_of(k, **over):
        e = engine(k, **over)
        b = e.export_state()
        e.close()
        return b

    second = dict(lam=0.5) if kind == "ppo" else dict(cg_iters=4)
    name = "grl_ppo_config\\.lam" if kind == "ppo" else "grl_trpo_config\\.cg_iters"
    snap = snapshot(eng)
    for bad, says in _refusals(eng, blob, blob_of(kind, gamma=0.9), blob_of(kind, **second), blob_of(other), name):
        with pytest.raises(GrlError, match=says):
            eng.import_state(bad)
        assert eng.lib.grl_ppo_state_import(eng.h, bad, len(bad)) == -1      # GRL_ERR_INVALID, every one of them
        assert_untouched(eng, snap, says)
    eng.import_state(blob)                                   # ... and its own blob still goes in
    assert_untouched(eng, snap, "own blob")
    # a blob written by grl_state_export (a handle that keeps no rollout)
    import checkpoint_util as scu
    sac = scu.SacRun(backend_factory, lib_path, extractor="mlp", B=16, n_replay=64).bare()
    with pytest.raises(GrlError, match="keeps no rollout"):
        eng.import_state(sac.export_state())
    assert_untouched(eng, snap, "SAC blob")
    sac.close(); eng.close()


def check_other_handles(backend_factory, lib_path):
    """grl_ppo_state_* on a SAC and a DQN handle: GRL_ERR_STATE, the message names the call, nothing moves."""
    import checkpoint_util as scu
    C = ctypes
    size = C.c_size_t()
    buf = C.create_string_buffer(64)
    for eng in (scu.SacRun(backend_factory, lib_path, extractor="mlp", B=16, n_replay=64).bare(),
                scu.QRun(backend_factory, lib_path, name="dqn").bare()):
        lib, h = eng.lib, eng.h
        before = words(eng, eng.state).copy()
        for name, call in (("grl_ppo_state_size", lambda: lib.grl_ppo_state_size(h, C.byref(size))),
                           ("grl_ppo_state_export", lambda: lib.grl_ppo_state_export(h, buf, 64)),
                           ("grl_ppo_state_import", lambda: lib.grl_ppo_state_import(h, buf, 64))):
            assert call() == -3, name                        # GRL_ERR_STATE
            assert name.encode() in lib.grl_last_error(), name
        assert np.array_equal(before, words(eng, eng.state))
        eng.close()


def check_load_state_checks_first(backend_factory, lib_path, tmp_path):
    """load_state refuses another configuration, the other kind of handle and a missing file with the engine untouched."""
    import pytest
    from grasp_rl._capi import GrlError

    def engine(k, **over):
        return make_engine(k, backend_factory, lib_path, normalize=2, **over)
    a = engine("ppo")
    Drive(a).rollout()
    a.save_state(str(tmp_path / "ck"))
    for other in (engine("ppo", n_steps=6), engine("ppo", lam=0.5), engine("trpo")):
        Drive(other).to("open")
        snap = snapshot(other)
        with pytest.raises(GrlError, match="differs|arena sizes|written by a PPO handle"):
            other.load_state(str(tmp_path / "ck"))
        assert_untouched(other, snap, "refused load_state")
        other.close()
    os.remove(str(tmp_path / "ck" / "replay_0.bin"))
    b = engine("ppo")
    snap = snapshot(b)
    with pytest.raises(GrlError, match="replay_0.bin is missing"):
        b.load_state(str(tmp_path / "ck"))
    assert_untouched(b, snap, "missing file")
    a.close(); b.close()


def check_interrupted_save(backend_factory, lib_path, tmp_path, monkeypatch):
    """os.rename fails once, between the two renames: load_state finds the previous checkpoint at <dir>.old."""
    import pytest
    path = str(tmp_path / "ck")
    a = make_engine("ppo", backend_factory, lib_path)
    d = Drive(a)
    d.rollout()
    a.save_state(path)
    first = snapshot(a)
    d.rollout()
    d.to("open")
    real, calls = os.rename, []

    def failing(src, dst):
        calls.append((src, dst))
        if len(calls) == 2:
            raise OSError("disk gone")
        return real(src, dst)

    monkeypatch.setattr(os, "rename", failing)
    with pytest.raises(OSError):
        a.save_state(path)
    monkeypatch.undo()
    assert not os.path.isdir(path) and os.path.isdir(path + ".old")
    b = make_engine("ppo", backend_factory, lib_path, params=False)
    b.load_state(path)
    now = snapshot(b)
    assert np.array_equal(now["state"], first["state"]) and np.array_equal(now["replay"], first["replay"]) and now["blob"] == first["blob"]
    a.close(); b.close()


# =================================================================================================== model level
def _unit(*key):
    return np.random.default_rng([int(k) for k in key])


class EpisodeEnv:
    def __init__(self, seed, start_episode=0):
        from grasp_rl.sb.spaces import Box
        self.observation_space = Box(-4.0, 4.0, shape=(OBS_DIM,), dtype=np.float32)
        self.action_space = Box(-1.0, 1.0, shape=(ACT_DIM,), dtype=np.float32)
        self.seed_, self.episode, self.t = int(seed), int(start_episode) - 1, 0
        self.fresh = False              # reset, and not stepped since
        self.actions = []

    def _obs(self):
        return (2.0 * _unit(self.seed_, self.episode, self.t, 0).standard_normal(OBS_DIM) + 0.5).astype(np.float32).clip(-4, 4)

    def reset(self):
        if not self.fresh:
            self.episode, self.t, self.fresh = self.episode + 1, 0, True
        return self._obs()

    def step(self, action):
        self.actions.append(np.array(action, np.float32).reshape(-1))
        self.t, self.fresh = self.t + 1, False
        rew = float(_unit(self.seed_, self.episode, self.t, 1).standard_normal()) - 0.1 * float(np.sum(np.square(action)))
        return self._obs(), rew, self.t >= EPISODE, {"episode": {"r": rew, "l": self.t}} if self.t >= EPISODE else {}


def make_env(n, start_episode=0, normalize=True):
    from grasp_rl.sb.vec_env import DummyVecEnv, VecNormalize
    venv = DummyVecEnv([(lambda i=i: EpisodeEnv(100 + i, start_episode)) for i in range(n)])
    return VecNormalize(venv, norm_obs=True, norm_reward=True, clip_obs=10.0) if normalize else venv


def install_emulation(lib):
    from grasp_rl.engine import PpoEngine, TrpoEngine
    from grasp_rl.sb.ppo2 import PPO2
    from grasp_rl.sb.trpo import TRPO
    from hostemu_backend import NumpyHostBackend
    PPO2._engine_factory = staticmethod(lambda cfg, ppo, device: PpoEngine(cfg, ppo, backend=NumpyHostBackend(), lib_path=lib))
    TRPO._engine_factory = staticmethod(lambda cfg, trpo, device: TrpoEngine(cfg, trpo, backend=NumpyHostBackend(), lib_path=lib))


def model_class(algo):
    from grasp_rl.sb import trpo
    from grasp_rl.sb.ppo2 import PPO2
    trpo.VF_BATCH = 4           # (a constant of stable-baselines, 128: 16-row batches would never fit the value tower)
    return PPO2 if algo == "ppo" else trpo.TRPO


def schedule(total, full):
    """3e-4 * f over `full` timesteps, as a learn of `total` timesteps sees it."""
    return (lambda f: 3e-4 * f) if total == full else (lambda f: 3e-4 * (1.0 - (1.0 - f) * total / full))


# algo, n_envs, the rollout, length of run A, where the checkpoint is taken (in on_step calls), what run B asks learn for, and
# the episode its fresh environments start at
CASES = {
    # 12 vectorised steps = two episodes of every sub-environment; the second rollout has four slots written and three closed
    "ppo-n4": dict(algo="ppo", n=4, n_steps=8, full=96, save_at=12, more=48, start_episode=2, device_norm=False),
    "ppo-n4-device_norm": dict(algo="ppo", n=4, n_steps=8, full=96, save_at=12, more=48, start_episode=2, device_norm=True),
    # num_timesteps == 48: the open slot is the last of its rollout, finish and the update come first after the restore
    "ppo-n1": dict(algo="ppo", n=1, n_steps=8, full=96, save_at=48, more=48, start_episode=8, device_norm=False),
    # 42 environment steps = seven episodes, in slot 10 of the third batch; num_timesteps stands at 32 there (it grows by a
    # batch after every update), so 64 more make the 96 of run A
    "trpo": dict(algo="trpo", n=1, n_steps=16, full=96, save_at=42, more=64, start_episode=7, device_norm=False),
    "trpo-device_norm": dict(algo="trpo", n=1, n_steps=16, full=96, save_at=42, more=64, start_episode=7, device_norm=True),
}


def new_model(case, env, total, full=None):
    c = CASES[case]
    full = c["full"] if full is None else full
    cls = model_class(c["algo"])
    arch = {"net_arch": [dict(vf=[8, 8], pi=[16])]}
    if c["algo"] == "ppo":
        return cls("MlpPolicy", env, n_steps=c["n_steps"], nminibatches=2, noptepochs=2, learning_rate=schedule(total, full),
                   policy_kwargs=arch, seed=3, device_norm=c["device_norm"])
    # (TRPO takes no schedule for vf_stepsize: it is a constant of the device plan)
    return cls("MlpPolicy", env, timesteps_per_batch=c["n_steps"], vf_iters=2, vf_stepsize=3e-4, cg_iters=3, policy_kwargs=arch, seed=3,
               device_norm=c["device_norm"])


def load_kwargs(case, total, full):
    c = CASES[case]
    kw = {"device_norm": c["device_norm"]}
    if c["algo"] == "ppo":
        kw["learning_rate"] = schedule(total, full)      # (a zip holds the schedule's first value only)
    return kw


def result(model, env, skip):
    """Everything the runs are compared on.  skip: vectorised steps before the boundary (their actions are left out)."""
    eng = model.engine
    eng.synchronize()
    venv = env.venv if hasattr(env, "venv") else env
    out = {"state": np.asarray(eng.be.to_host(eng.state)).view(np.uint32).copy(),
           "vecnormalize": np.frombuffer(pickle.dumps(env if hasattr(env, "venv") else None), np.uint8),
           "counters": np.array([model.num_timesteps, getattr(model, "n_updates", 0)], np.int64),
           "actions": np.stack([np.stack(e.actions[skip:]) for e in venv.envs])}
    for k, v in model.get_parameters().items():
        out["p:" + k] = np.asarray(v, np.float32).reshape(-1).view(np.uint32)
    return out


class SaveAt:
    """Callback: calls `save(model)` in the on_step call number `at` and lets the run go on."""

    def __init__(self, at, save):
        self.at, self.save, self.calls, self.saved_at = at, save, 0, None

    def __call__(self, locals_, globals_):
        self.calls += 1
        if self.calls == self.at:
            model = locals_["self"]
            self.saved_at = model.num_timesteps
            self.save(model)
        return True


def saver(how, path, include_replay=True):
    if how == "checkpoint":
        return lambda model: model.save_checkpoint(path, include_replay=include_replay)

    def plain(model):                           # the drop-in route: plain save behind the switch
        os.environ["GRL_CHECKPOINT_STATE"] = "1"
        try:
            model.save(path)
        finally:
            del os.environ["GRL_CHECKPOINT_STATE"]
    return plain


def run_a(case, tmp_path, how="checkpoint"):
    """learn(full) with a checkpoint on the way; returns (result, path of the checkpoint)."""
    c = CASES[case]
    env = make_env(c["n"])
    model = new_model(case, env, c["full"])
    path = os.path.join(str(tmp_path), "model_" + how)
    cb = SaveAt(c["save_at"], saver(how, path))
    model.learn(c["full"], callback=cb)
    assert cb.saved_at is not None and model.num_timesteps == c["full"]
    if c["algo"] == "ppo":
        assert cb.saved_at == c["save_at"] * c["n"]
    assert os.path.isfile(path + ".zip") and os.path.isfile(os.path.join(path + ".state", "host.pkl"))
    out = result(model, env, c["save_at"])
    model.engine.close()
    return out, path


def run_child(spec, tmp_path, environ_extra=None):
    environ = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    environ.pop("GRL_CHECKPOINT_STATE", None)
    environ.update(environ_extra or {})
    spec = dict(spec, out=os.path.join(str(tmp_path), "b_%s.npz" % spec["how"]))
    spec_file = os.path.join(str(tmp_path), "spec_%s.json" % spec["how"])
    with open(spec_file, "w") as f:
        json.dump(spec, f)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), spec_file], env=environ, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(spec["out"]) as z:
        return {k: z[k] for k in z.files}


def run_b(case, path, tmp_path, lib, how="checkpoint"):
    """A fresh process: restore, learn(more, reset_num_timesteps=False), the result."""
    c = CASES[case]
    spec = {"case": case, "how": how, "path": path, "lib": lib, "total": c["full"], "full": c["full"], "more": c["more"], "start_episode": c["start_episode"]}
    return run_child(spec, tmp_path, {"GRL_CHECKPOINT_STATE": "1"} if how == "save" else None)


def run_returned(case, tmp_path, lib, T):
    """learn(T) -> save_checkpoint -> a fresh process -> load_checkpoint -> learn(T, reset_num_timesteps=False)."""
    c = CASES[case]
    env = make_env(c["n"])
    model = new_model(case, env, T, full=2 * T)
    model.learn(T)
    path = os.path.join(str(tmp_path), "returned")
    model.save_checkpoint(path)
    model.engine.close()
    spec = {"case": case, "how": "checkpoint", "path": path, "lib": lib, "total": T, "full": 2 * T, "more": T, "start_episode": T // (c["n"] * EPISODE)}
    return run_child(spec, tmp_path)


def resume_and_finish(spec):
    if spec["lib"]:
        install_emulation(spec["lib"])
    case = spec["case"]
    c = CASES[case]
    env = make_env(c["n"], start_episode=spec["start_episode"])
    cls = model_class(c["algo"])
    load = cls.load_checkpoint if spec["how"] == "checkpoint" else cls.load      # "save": GRL_CHECKPOINT_STATE=1 is in the environment
    model = load(spec["path"], env, **load_kwargs(case, spec["total"], spec["full"]))
    assert model._resume is not None
    model.learn(spec["more"], reset_num_timesteps=False)
    np.savez(spec["out"], **result(model, env, 0))


def assert_equal_runs(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), \
            "%s differs in %d of %d words" % (k, int(np.sum(a[k] != b[k])) if a[k].shape == b[k].shape else -1, a[k].size)


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        resume_and_finish(json.load(f))
