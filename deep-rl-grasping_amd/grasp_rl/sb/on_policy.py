"""``OnPolicyModel``: what ``PPO2`` and ``TRPO`` share beyond ``BaseModel`` -- the actor-critic ``MlpPolicy`` both device plans
build (``_net_arch``, the Box checks), acting, the VecNormalize observation statistics on the device, the frame of ``learn`` around
the class's own ``_learn_loop``, and the host half of a checkpoint: the record of the rollout in progress and the seam of a
continued run.  Each class keeps its constructor, the algorithm part of ``setup_model``, ``_learn_loop``,
``_SAVED`` and the contents of its zip.
"""
from collections import deque

import numpy as np

from .. import _capi
from . import logger
from . import spaces as sp
from .base import BaseModel, resolve_device_norm
from .callbacks import as_callback
from .checkpoint import _common_state, _restore_common


def explained_variance(y_pred, y_true):
    var_y = np.var(y_true)
    return np.nan if var_y == 0 else 1.0 - np.var(y_true - y_pred) / var_y


def _safe_mean(xs):
    return np.nan if len(xs) == 0 else float(np.mean(xs))


def _normalize_kwargs(vn):
    """make_ppo_config / make_trpo_config: a handle that can keep the wrapper's observation statistics (normalize = 2)."""
    if vn is None or not vn.norm_obs:
        return {}
    return dict(normalize=2, clip_obs=float(vn.clip_obs), norm_eps=float(vn.epsilon))


def _episodes(infos):
    return [info["episode"] for info in infos if isinstance(info, dict) and info.get("episode") is not None]


class OnPolicyModel(BaseModel):
    _loop = None           # the running (or last) learn's record of its rollout: what a checkpoint keeps of the host loop

    # ------------------------------------------------------------------ model
    def _net_arch(self):
        """(pi widths, vf widths) of policy_kwargs; refuses what the device plan does not build."""
        cls = type(self).__name__
        pol = self.policy
        name = getattr(pol, "__name__", str(pol))
        if isinstance(pol, str):
            if pol != "MlpPolicy":
                raise NotImplementedError("%s: policy %r is not implemented (only the actor-critic MlpPolicy)" % (cls, pol))
        elif getattr(pol, "feature_extraction", "mlp") == "cnn" or "Lstm" in name or "Cnn" in name:
            raise NotImplementedError("%s: policy %s is not implemented (only the actor-critic MlpPolicy: CnnPolicy, "
                                      "MlpLstmPolicy and their relatives are refused)" % (cls, name))
        kw = self.policy_kwargs
        act_fun = kw.get("act_fun")
        if act_fun is not None and getattr(act_fun, "__name__", str(act_fun)) != "tanh":
            raise NotImplementedError("%s: act_fun %s is not implemented (the towers' activation is tanh)"
                                      % (cls, getattr(act_fun, "__name__", act_fun)))
        unknown = sorted(set(kw) - {"net_arch", "act_fun", "feature_extraction"})
        if unknown:
            raise NotImplementedError("%s: policy_kwargs %s are not implemented" % (cls, unknown))
        if kw.get("feature_extraction", "mlp") != "mlp":
            raise NotImplementedError("%s: feature_extraction %r is not implemented" % (cls, kw["feature_extraction"]))
        arch = kw.get("net_arch")
        if arch is None:
            return (64, 64), (64, 64)
        arch = list(arch)
        if len(arch) != 1 or not isinstance(arch[0], dict):
            raise NotImplementedError("%s: shared layers in net_arch are not implemented (net_arch must be "
                                      "[dict(vf=[...], pi=[...])], got %r)" % (cls, arch))
        pi, vf = tuple(int(w) for w in arch[0].get("pi", ())), tuple(int(w) for w in arch[0].get("vf", ()))
        for nm, t in (("pi", pi), ("vf", vf)):
            if not 1 <= len(t) <= _capi.GRL_MAX_LAYERS or any(not 1 <= w <= 1024 for w in t):
                raise NotImplementedError("%s: the %s tower needs 1..%d layers of widths 1..1024, got %r"
                                          % (cls, nm, _capi.GRL_MAX_LAYERS, list(t)))
        return pi, vf

    def _check_spaces(self):
        """The head of ``setup_model``: Box actions, Box observations of any rank (flattened in C order); sets the two sizes."""
        if not sp.is_box(self.action_space):
            raise NotImplementedError("%s: %s action spaces are not implemented (Box only; Discrete / MultiDiscrete are refused)"
                                      % (type(self).__name__, type(self.action_space).__name__))
        if not sp.is_box(self.observation_space) or len(tuple(self.observation_space.shape)) < 1:
            raise ValueError("Box observations expected, got %s" % (self.observation_space,))
        self._obs_dim = int(np.prod(tuple(self.observation_space.shape)))
        self._act_dim = int(np.prod(tuple(self.action_space.shape)))

    # ------------------------------------------------------------------ acting
    def _clip(self, actions):
        return np.clip(actions, self.action_space.low, self.action_space.high)

    def predict(self, observation, state=None, mask=None, deterministic=False):
        observation = np.asarray(observation)
        single = observation.shape == tuple(self.observation_space.shape)
        obs = np.asarray(observation, np.float32).reshape(-1, self._obs_dim)
        cap = self.engine.n_envs
        acts = np.concatenate([self.engine.act(obs[k:k + cap], deterministic=deterministic) for k in range(0, obs.shape[0], cap)])
        acts = self._clip(acts.reshape((-1,) + tuple(self.action_space.shape)))
        return (acts[0] if single else acts), None

    # ------------------------------------------------------------------ learn
    def _learn(self, total_timesteps, callback, log_interval, tb_log_name, reset_num_timesteps):
        """``learn`` of both classes, around the class's own ``_learn_loop``."""
        total_timesteps, resume = self._begin_learn(total_timesteps, reset_num_timesteps)
        device_norm = self._resolve_device_norm(callback)      # (decided from the callback the USER handed over)
        callback = as_callback(callback)
        callback.init_callback(self)
        # stable-baselines hands callbacks a FileWriter when tensorboard_log is set, None otherwise
        writer = logger.SummaryWriter(self.tensorboard_log, tb_log_name) if self.tensorboard_log else None
        try:
            self._attach_device_norm(device_norm, upload=resume is None)      # restored: the device holds the statistics already
            self._learn_loop(total_timesteps, callback, log_interval, writer, resume)
        finally:
            self._detach_device_norm()
            if writer is not None:
                writer.close()
        return self

    # ------------------------------------------------------------------ VecNormalize observation statistics on the device
    def _resolve_device_norm(self, user_callback):
        return self.device_norm is not False and resolve_device_norm(self.device_norm, user_callback, None, None)

    def _attach_device_norm(self, device_norm, upload=True):
        vn = self._vec_normalize_env
        if not device_norm or vn is None or not vn.norm_obs:
            return
        if self.engine.cfg.normalize == 2:
            if not upload:      # ... unless the saved run kept them on the host: then the wrapper's restored copy is the newer one
                mean, var, count = self.engine.get_obs_stats(tuple(vn.obs_rms.mean.shape))
                upload = not (np.array_equal(mean, vn.obs_rms.mean) and np.array_equal(var, vn.obs_rms.var) and count == vn.obs_rms.count)
            vn.attach_device(self.engine, upload=upload)
        else:      # a zip loaded without env and given a normalised env later: the device plan holds no statistics
            logger.warn("%s: device_norm needs a model built on the VecNormalize env (pass env= to the constructor or to load); "
                        "this one was built without it -> VecNormalize stays on the host" % type(self).__name__)

    def _detach_device_norm(self):
        vn = self._vec_normalize_env
        if vn is not None and vn._dev is not None:      # whatever ended the loop: the wrapper carries the statistics again
            vn.detach_device()

    def _rows(self, obs, n):
        """What ``engine.step`` / ``engine.finish`` get for the observations in hand: None when the wrapper's latest
        ``engine.observe`` uploaded exactly them (the device normalised them with the statistics of that moment, as the host
        path would have), else the array -- a callback cleared ``training``, the host path, or no wrapper at all."""
        vn = self._vec_normalize_env
        if vn is not None and vn._dev is self.engine and vn.observed_serial is not None \
                and vn.observed_serial == getattr(self.engine, "_observe_serial", None):
            return None
        return obs.reshape(n, -1)

    # ------------------------------------------------------------------ checkpoint / resume (sb/checkpoint.py)
    def _loop_snapshot(self, include_replay=True):
        """What the loop holds between two engine calls, as host.pkl keeps it (None before the first ``learn``).  A callback
        saves between ``engine.step`` and ``engine.rewards``: the slot is then written and not closed, its rewards are in
        ``rewards`` already and its infos have not been looked at yet -- their episodes are taken in here."""
        lp = self._loop
        if lp is None:
            return None
        written, closed, _ = self.engine.rollout_cursor()
        out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in lp.items() if k not in ("infos", "ep_infos")}
        out["ep_infos"] = list(lp["ep_infos"]) + (_episodes(lp["infos"]) if written == closed + 1 else [])
        return out

    def _host_extra(self):
        return {}

    def _set_host_extra(self, extra):
        pass

    def _host_state(self, include_replay):
        """host.pkl of a PPO2 / TRPO model: the format number and the keys every model writes, then what these loops keep.
        ``loop`` is the model's own record of the rollout in progress (``_loop_snapshot``: the flags the next step or finish takes,
        the rewards of a slot that is written and not closed, the episode infos and value / reward rows collected so far, the index
        of the update in progress; TRPO: its generator's counters), ``extra`` what else the model class carries."""
        st = _common_state(self, include_replay)
        # (n_updates is PPO2's: TRPO counts its iterations in the loop record, and its host.pkl says 0)
        st.update(n_updates=int(getattr(self, "n_updates", 0)), rng=self._rng.get_state(),      # np.random.RandomState: the permutations
                  ep_info_buf=list(self.ep_info_buf), loop=self._loop_snapshot(include_replay), extra=self._host_extra())
        return st

    def _restore_host_state(self, st):
        """The host half of a restore (the engine is loaded): counters, the permutation generator, episode statistics,
        VecNormalize, and the record of the rollout in progress for the next ``learn(reset_num_timesteps=False)``."""
        self._resume = dict(_restore_common(self, st), loop=st["loop"])
        if hasattr(self, "n_updates"):
            self.n_updates = st["n_updates"]
        self._rng = np.random.RandomState()
        self._rng.set_state(st["rng"])
        self.ep_info_buf = deque(st["ep_info_buf"], maxlen=100)
        self._set_host_extra(st["extra"])
        self._loop = None

    def _resumed_start(self, resume):
        """The seam of a continued run: (observations, cursor, the saved loop record or None).  The environment is the one thing
        a checkpoint cannot hold: it is reset ONCE, its first observations normalised with the restored statistics and not
        counted into them (``reset_restored``; device path: uploaded without a statistics update), and every sub-environment
        starts an episode -- the caller's flags are 1 whatever the checkpoint says, so neither the value bootstrap nor GAE
        crosses the seam.  The record is None when the rollout stayed out of the checkpoint (an empty one starts here)."""
        vn, eng = self._vec_normalize_env, self.engine
        obs = np.asarray(vn.reset_restored(resume["ret"]) if vn is not None else self.env.reset(), np.float32)
        written, closed, finished = eng.rollout_cursor()
        saved = resume["loop"]
        if written > 0 and (saved is None or "rewards" not in saved):      # (a rollout no learn of this class wrote)
            eng.reset_rollout()
            written = closed = 0
        return obs, (written, closed, finished), (saved if written > 0 else None)

    # ------------------------------------------------------------------ persistence
    def _before_setup(self, data, params):
        self._rng = np.random.RandomState(self.seed)
        if "net_arch" not in self.policy_kwargs:      # the towers as the parameters describe them
            def widths(nm):
                out, l = [], 0
                while "model/%s_fc%d/w:0" % (nm, l) in params:
                    out.append(int(params["model/%s_fc%d/w:0" % (nm, l)].shape[1]))
                    l += 1
                return out
            if (widths("pi"), widths("vf")) != ([64, 64], [64, 64]):
                self.policy_kwargs["net_arch"] = [dict(vf=widths("vf"), pi=widths("pi"))]
