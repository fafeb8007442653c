"""Full-state checkpoints of the ``SAC`` / ``DQN`` / ``BDQ`` / ``PPO2`` / ``TRPO`` models: the
stable-baselines zip plus, next to it, a directory with the engine's training state (``engine.save_state``: parameters, optimiser
moments and counters, device RNG position, running statistics, replay ring, priorities -- PPO2 / TRPO: the rollout) and
``host.pkl``, the few things this host loop keeps itself: ``num_timesteps``, ``n_updates``, the exploration generator, the
schedules' reference length, the VecNormalize statistics and returns -- PPO2 / TRPO: the permutation generator, the index of the
update in progress and what the loop holds between two engine calls (``OnPolicyModel._host_state``).  A model restored from it
continues with ``learn(n, reset_num_timesteps=False)`` as if ``learn`` had never returned.

``model.save_checkpoint(path)`` / ``Model.load_checkpoint(path, env)`` do this explicitly.  For scripts that only know
``model.save`` / ``Model.load`` -- the reference's callbacks and its ``--load_dir`` -- GRL_CHECKPOINT_STATE=1 makes ``save``
write the directory too and ``load`` restore from it when it is there; GRL_CHECKPOINT_REPLAY=0 leaves the ring out.  The
directory of ``<p>`` or ``<p>.zip`` is ``<p>.state``; one replica of a data-parallel job writes ``<p>.state.rank<k>`` (replay
shards and priority trees are per rank).
"""
import os
import pickle

import numpy as np

from .._capi import GrlError

HOST_FILE = "host.pkl"
HOST_FORMAT = 1


def enabled():
    return os.environ.get("GRL_CHECKPOINT_STATE", "0") == "1"


def with_replay():
    return os.environ.get("GRL_CHECKPOINT_REPLAY", "1") != "0"


def state_dir(path, rt=None):
    path = os.fspath(path)
    base = path[:-4] if path.endswith(".zip") else path
    return base + ".state" + ("" if rt is None else ".rank%d" % rt.rank)


def _space_rng(space):
    """(attribute name, generator) of this package's spaces (`_rng`) or gym's (`np_random`)."""
    for name in ("_rng", "np_random"):
        gen = space.__dict__.get(name) if hasattr(space, "__dict__") else None
        if gen is not None:
            return name, gen
    return None


def _rms_state(rms):
    return {"mean": np.array(rms.mean, np.float64), "var": np.array(rms.var, np.float64), "count": rms.count}     # count: type kept


def _vn_state(vn):
    vn.pull_device_stats()          # attached: the device holds the observation statistics
    return {"obs_rms": _rms_state(vn.obs_rms), "ret_rms": _rms_state(vn.ret_rms),
            "ret": np.array(vn.ret, np.float64), "clip_obs": vn.clip_obs, "clip_reward": vn.clip_reward,
            "gamma": vn.gamma, "epsilon": vn.epsilon, "norm_obs": vn.norm_obs, "norm_reward": vn.norm_reward}


def _vn_restore(vn, vs):
    for rms, s in ((vn.obs_rms, vs["obs_rms"]), (vn.ret_rms, vs["ret_rms"])):
        rms.mean, rms.var, rms.count = s["mean"].copy(), s["var"].copy(), s["count"]
    vn.ret = vs["ret"].copy()
    vn.clip_obs, vn.clip_reward = vs["clip_obs"], vs["clip_reward"]


def _common_state(model, include_replay):
    """The keys of host.pkl that every model class writes: those ``_read_host`` checks, the step counter, what the schedules
    measure their progress against, and the VecNormalize statistics."""
    rt, vn = model._dp_rt, model._vec_normalize_env
    return {"format": HOST_FORMAT, "model": type(model).__name__, "world": 1 if rt is None else rt.world,
            "include_replay": bool(include_replay), "num_timesteps": int(model.num_timesteps),
            "schedule_total": model._schedule_total, "vec_normalize": None if vn is None else _vn_state(vn)}


def _restore_common(model, st):
    """Puts back what ``_common_state`` took; returns the start of the model's ``_resume`` record."""
    model.num_timesteps = st["num_timesteps"]
    vn, vs = model._vec_normalize_env, st["vec_normalize"]
    if vn is not None:
        _vn_restore(vn, vs)
    return {"schedule_total": st["schedule_total"], "ret": None if vs is None else vs["ret"].copy()}


def write_state(model, path, include_replay=True):
    """The engine directory with host.pkl inside, one atomic step (engine.save_state)."""
    d = state_dir(path, model._dp_rt)
    model.engine.save_state(d, include_replay=include_replay,
                            extra={HOST_FILE: pickle.dumps(model._host_state(include_replay), protocol=4)})
    return d


def _find(path, rt):
    d = state_dir(path, rt)
    if not os.path.isdir(d) and os.path.isdir(d + ".old"):       # a save died between its two renames
        d += ".old"
    return d if os.path.isdir(d) else None


def _read_host(model, d):
    with open(os.path.join(d, HOST_FILE), "rb") as f:
        st = pickle.load(f)
    if st.get("format") != HOST_FORMAT:
        raise GrlError("checkpoint host state has format %r, this build reads %d" % (st.get("format"), HOST_FORMAT))
    if st.get("model") != type(model).__name__:
        raise GrlError("checkpoint of a %s model loaded into %s" % (st.get("model"), type(model).__name__))
    world = 1 if model._dp_rt is None else model._dp_rt.world
    if st.get("world") != world:
        raise GrlError("checkpoint was written by a job of %r replicas, this one has %d" % (st.get("world"), world))
    vs, vn = st.get("vec_normalize"), model._vec_normalize_env
    if (vs is None) != (vn is None):
        raise GrlError("checkpoint was written %s VecNormalize, the env given now is %s one"
                       % (("with", "without") if vs is not None else ("without", "with")))
    if vs is not None and (tuple(vs["obs_rms"]["mean"].shape) != tuple(vn.obs_rms.mean.shape) or len(vs["ret"]) != vn.num_envs):
        raise GrlError("checkpoint VecNormalize state does not fit the env (observation shape or number of envs)")
    return st


def restore_state(model, path, required):
    """Restores engine and host state of `model` (built from the zip at `path`, env set) from the directory next to it.
    Returns False when there is none and it is not `required`.  Data parallel: COLLECTIVE -- every rank reads and checks its
    own directory first, then all vote (parallel.vote_all) and only a unanimous job imports; otherwise every rank raises."""
    rt = model._dp_rt
    d, st, why = _find(path, rt), None, None
    if d is None:
        why = "no checkpoint state at %s" % state_dir(path, rt)
    else:
        try:
            st = _read_host(model, d)
        except (OSError, pickle.UnpicklingError, EOFError, KeyError, GrlError) as e:
            why = "%s: %s" % (d, e)
    if rt is not None:
        from ..parallel import vote_all
        present = vote_all(d is not None, rt.ctrl)
        absent = vote_all(d is None, rt.ctrl)
        if absent and not required:
            return False
        if not vote_all(st is not None, rt.ctrl):
            raise GrlError(why or ("rank %d read its checkpoint, another replica could not read its own%s"
                                   % (rt.rank, "" if present else " (not every rank has a state directory)")))
    elif st is None:
        if d is None and not required:
            return False
        raise GrlError(why)
    model.engine.load_state(d)
    model._restore_host_state(st)
    return True


def _refuse_other_model(cls, path):
    """Before the zip is read: a state directory written by another model class is refused by name (its zip need not even hold
    this class's parameters)."""
    d = _find(path, None)
    if d is None:
        return
    try:
        with open(os.path.join(d, HOST_FILE), "rb") as f:
            name = pickle.load(f).get("model")
    except (OSError, pickle.UnpicklingError, EOFError, AttributeError):
        return          # restore_state says what is wrong with it
    if name != cls.__name__:
        raise GrlError("checkpoint of a %s model loaded into %s" % (name, cls.__name__))


class CheckpointMixin:
    """save_checkpoint / load_checkpoint and the GRL_CHECKPOINT_STATE hooks of save / load.  The model class provides
    ``_save_zip(path)`` and ``_load_zip(path, env, ...)``, and fills in or replaces ``_host_state`` / ``_restore_host_state``."""
    _resume = None
    _schedule_total = None

    def save_checkpoint(self, path, include_replay=True):
        """The ordinary zip at `path` (rank 0 of a data-parallel job: the replicas' parameters are equal) and the full
        training state in the directory next to it (every rank its own)."""
        rt = self._dp_rt
        out = self._save_zip(path) if rt is None or rt.rank == 0 else path
        write_state(self, path, include_replay)
        if rt is not None:
            rt.barrier()
        return out

    @classmethod
    def load_checkpoint(cls, path, env=None, **kwargs):
        _refuse_other_model(cls, path)
        model = cls._load_zip(path, env=env, **kwargs)
        restore_state(model, path, required=True)
        return model

    def save(self, save_path, cloudpickle=False):
        out = self._save_zip(save_path)
        if enabled() and isinstance(save_path, (str, os.PathLike)):
            write_state(self, save_path, with_replay())
        return out

    @classmethod
    def load(cls, load_path, env=None, custom_objects=None, **kwargs):
        model = cls._load_zip(load_path, env=env, custom_objects=custom_objects, **kwargs)
        if enabled() and isinstance(load_path, (str, os.PathLike)):
            restore_state(model, load_path, required=False)
        return model

    def _take_resume(self, reset_num_timesteps):
        """The restored position for a learn() that continues (None otherwise); a checkpoint is continued once."""
        resume, self._resume = (None if reset_num_timesteps else self._resume), None
        return resume

    # ------------------------------------------------------------------ host.pkl: the off-policy models; OnPolicyModel has its own
    def _host_state(self, include_replay):
        """host.pkl of a SAC / DQN / BDQ model.  ``max_priority`` and ``exploration_eps`` are the Q models' to fill, ``ent_init``
        is SAC's; every class writes all the keys."""
        st = _common_state(self, include_replay)
        st.update(n_updates=int(self.n_updates), rng=self._rng.bit_generator.state, max_priority=None, exploration_eps=None,
                  ent_init=None, action_space_rng=None)
        gen = _space_rng(self.action_space)       # the learning_starts phase samples from the space's own generator
        if gen is not None:
            st["action_space_rng"] = (gen[0], pickle.dumps(gen[1]))
        return st

    def _restore_host_state(self, st):
        """The host half of a restore (the engine is loaded)."""
        # consumed by the next learn(reset_num_timesteps=False): continue in place (no reset statistics, no new schedules)
        self._resume = _restore_common(self, st)
        self.n_updates = st["n_updates"]
        self._rng = np.random.default_rng()
        self._rng.bit_generator.state = st["rng"]
        if st["action_space_rng"] is not None and hasattr(self.action_space, st["action_space_rng"][0]):
            setattr(self.action_space, st["action_space_rng"][0], pickle.loads(st["action_space_rng"][1]))
