"""Full-state checkpoints of the ``SAC`` / ``DQN`` / ``BDQ`` / ``PPO2`` / ``TRPO`` models: the
stable-baselines zip plus, next to it, a directory with the engine's training state (``engine.save_state``: parameters, optimiser
moments and counters, device RNG position, running statistics, replay ring, priorities -- PPO2 / TRPO: the rollout) and
``host.pkl``, the few things this host loop keeps itself: ``num_timesteps``, ``n_updates``, the exploration generator, the
schedules' reference length, the VecNormalize statistics and returns -- PPO2 / TRPO: the permutation generator, the index of the
update in progress and what the loop holds between two engine calls (``_on_policy_host_state``).  A model restored from it
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


def _on_policy_host_state(model, include_replay):
    """host.pkl of a PPO2 / TRPO model: the same format number and the keys ``_read_host`` checks, then what these loops keep.
    ``loop`` is the model's own record of the rollout in progress (``_loop_snapshot``: the flags the next step or finish takes,
    the rewards of a slot that is written and not closed, the episode infos and value / reward rows collected so far, the index
    of the update in progress; TRPO: its generator's counters), ``extra`` what else the model class carries."""
    vn = model._vec_normalize_env
    return {"format": HOST_FORMAT, "model": type(model).__name__, "world": 1, "include_replay": bool(include_replay),
            "num_timesteps": int(model.num_timesteps), "n_updates": int(getattr(model, "n_updates", 0)),
            "rng": model._rng.get_state(),          # np.random.RandomState: draws the permutations
            "schedule_total": model._schedule_total, "ep_info_buf": list(model.ep_info_buf),
            "vec_normalize": None if vn is None else _vn_state(vn),
            "loop": model._loop_snapshot(include_replay), "extra": model._host_extra()}


def host_state(model, include_replay):
    if getattr(model, "_on_policy", False):
        return _on_policy_host_state(model, include_replay)
    rt = model._dp_rt
    st = {"format": HOST_FORMAT, "model": type(model).__name__, "world": 1 if rt is None else rt.world,
          "include_replay": bool(include_replay), "num_timesteps": int(model.num_timesteps), "n_updates": int(model.n_updates),
          "rng": model._rng.bit_generator.state, "max_priority": getattr(model, "_max_priority", None),
          # what the exploration / beta / learning-rate schedules measure their progress against, and where they stand
          "schedule_total": getattr(model, "_schedule_total", None),
          "exploration_eps": None if getattr(model, "exploration", None) is None
          else float(model.exploration.value(model.num_timesteps)),
          "ent_init": getattr(model, "_ent_init", None), "action_space_rng": None, "vec_normalize": None}
    gen = _space_rng(model.action_space)       # the learning_starts phase samples from the space's own generator
    if gen is not None:
        st["action_space_rng"] = (gen[0], pickle.dumps(gen[1]))
    vn = model._vec_normalize_env
    if vn is not None:
        st["vec_normalize"] = _vn_state(vn)
    return st


def write_state(model, path, include_replay=True):
    """The engine directory with host.pkl inside, one atomic step (engine.save_state)."""
    d = state_dir(path, model._dp_rt)
    model.engine.save_state(d, include_replay=include_replay,
                            extra={HOST_FILE: pickle.dumps(host_state(model, include_replay), protocol=4)})
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
    if getattr(model, "_on_policy", False):
        return _restore_on_policy(model, st)
    model.num_timesteps, model.n_updates = st["num_timesteps"], st["n_updates"]
    model._rng = np.random.default_rng()
    model._rng.bit_generator.state = st["rng"]
    if st["max_priority"] is not None:
        model._max_priority = st["max_priority"]
    if st["ent_init"] is not None:
        model._ent_init = st["ent_init"]
    if st["action_space_rng"] is not None and hasattr(model.action_space, st["action_space_rng"][0]):
        setattr(model.action_space, st["action_space_rng"][0], pickle.loads(st["action_space_rng"][1]))
    vn, vs = model._vec_normalize_env, st["vec_normalize"]
    if vn is not None:
        _vn_restore(vn, vs)
    # consumed by the next learn(reset_num_timesteps=False): continue in place (no reset statistics, no new schedules)
    model._resume = {"schedule_total": st["schedule_total"], "ret": None if vs is None else vs["ret"].copy()}
    model._restored_norm_stamp()
    return True


def _restore_on_policy(model, st):
    """The host half of a PPO2 / TRPO restore (the engine is loaded): counters, the permutation generator, episode statistics,
    VecNormalize, and the record of the rollout in progress for the next ``learn(reset_num_timesteps=False)``."""
    from collections import deque
    model.num_timesteps = st["num_timesteps"]
    if hasattr(model, "n_updates"):
        model.n_updates = st["n_updates"]
    model._rng = np.random.RandomState()
    model._rng.set_state(st["rng"])
    model.ep_info_buf = deque(st["ep_info_buf"], maxlen=100)
    vn, vs = model._vec_normalize_env, st["vec_normalize"]
    if vn is not None:
        _vn_restore(vn, vs)
    model._set_host_extra(st["extra"])
    model._loop = None
    model._resume = {"schedule_total": st["schedule_total"], "ret": None if vs is None else vs["ret"].copy(), "loop": st["loop"]}
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
    ``_save_zip(path)``, ``_load_zip(path, env, ...)`` and ``_restored_norm_stamp()``."""
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

    def _restored_norm_stamp(self):
        pass
