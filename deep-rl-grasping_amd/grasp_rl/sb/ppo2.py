"""``PPO2`` with the constructor / learn / predict / save / load surface the reference uses
(/root/reference/manipulation_main/training/sb_helper.py:137-154 ``sb.PPO2(MlpPolicy, env, verbose=2, gamma=...,
learning_rate=..., tensorboard_log=...)``; loader at train_stable_baselines.py:99-100).

Everything that touches a tensor runs in the HIP engine (``PpoEngine``; csrc/plan_ppo.inl, csrc/ppo_kernels.h): the policy
step writes observation, action, value and neglogp straight into the rollout on the device, GAE and the
``noptepochs * nminibatches`` clipped updates read it there.  This file is the host loop of stable-baselines 2.10.1
``PPO2.learn`` / ``Runner._run``: the env steps (actions clipped to the space for the env only), the callback protocol, one
permutation per epoch from the model's seeded generator, episode statistics and the logger.

Scope: the actor-critic ``MlpPolicy`` (two tanh towers, ``net_arch=[dict(vf=[...], pi=[...])]``) on ``Box`` actions, observations
of any rank flattened in C order and not divided by 255, N environments (a VecEnv, or GRL_NUM_ENVS around the script's
one-factory DummyVecEnv).  Everything else says what it refuses.  ``model.save`` writes the stable-baselines zip only;
``save_checkpoint`` / ``load_checkpoint`` -- or GRL_CHECKPOINT_STATE=1 behind ``save`` / ``load`` -- keep the full training state
next to it (sb/checkpoint.py), and ``learn(n, reset_num_timesteps=False)`` on a restored model continues the rollout that was
in progress (``_resumed_start``: the open slot, the seam).

VecNormalize: stable-baselines normalises a PPO observation once, at step time, with the statistics right after that step's
update, and the rollout stores the normalised row.  By default the wrapper does that on the host.  ``device_norm=True`` (or
GRL_DEVICE_NORM=1 / auto; unset means off) keeps the OBSERVATION statistics in device memory while ``learn`` runs: every env step
uploads the raw observations once (``engine.observe``: one launch updates the statistics and writes the normalised rows) and
``step`` / ``finish`` read those rows -- the same bits as the host path, float64 statistics included; the wrapper carries them
again when ``learn`` returns.  Rewards are normalised on the host in both cases (n_envs floats per step); callbacks see raw
observations in ``locals`` while the device path is on, which is why ``'auto'`` leaves it off for a callback that may read them.
"""
import time
from collections import deque

import numpy as np

from .. import _capi
from ..engine import PpoEngine
from ..init import init_ppo_parameters
from . import logger
from . import save_util
from . import spaces as sp
from .callbacks import as_callback
from .checkpoint import CheckpointMixin
from .vec_env import DummyVecEnv, VecEnv, expand_training_env, unwrap_vec_normalize


def _constfn(v):
    return v if callable(v) else (lambda _frac: float(v))


def explained_variance(y_pred, y_true):
    var_y = np.var(y_true)
    return np.nan if var_y == 0 else 1.0 - np.var(y_true - y_pred) / var_y


def _safe_mean(xs):
    return np.nan if len(xs) == 0 else float(np.mean(xs))


def _device_norm_setting(device_norm):
    """The ``device_norm`` keyword of PPO2 / TRPO: True, False or 'auto'; None reads GRL_DEVICE_NORM with the DQN / BDQ rule (unset
    means off, 1 on, auto auto)."""
    import os
    if device_norm is None:
        device_norm = {"0": False, "1": True, "auto": "auto"}.get(os.environ.get("GRL_DEVICE_NORM", "0"), False)
    return device_norm if device_norm == "auto" else bool(device_norm)


def _normalize_kwargs(vn):
    """make_ppo_config / make_trpo_config: a handle that can keep the wrapper's observation statistics (normalize = 2)."""
    if vn is None or not vn.norm_obs:
        return {}
    return dict(normalize=2, clip_obs=float(vn.clip_obs), norm_eps=float(vn.epsilon))


def _episodes(infos):
    return [info["episode"] for info in infos if isinstance(info, dict) and info.get("episode") is not None]


class PPO2(CheckpointMixin):
    _on_policy = True      # sb/checkpoint.py: host.pkl of the on-policy models
    _dp_rt = None          # one replica
    _loop = None           # the running (or last) learn's record of its rollout: what a checkpoint keeps of the host loop
    _engine_factory = staticmethod(lambda cfg, ppo, device: PpoEngine(cfg, ppo, device=device))

    def __init__(self, policy, env, gamma=0.99, n_steps=128, ent_coef=0.01, learning_rate=2.5e-4, vf_coef=0.5,
                 max_grad_norm=0.5, lam=0.95, nminibatches=4, noptepochs=4, cliprange=0.2, cliprange_vf=None, verbose=0,
                 tensorboard_log=None, _init_setup_model=True, policy_kwargs=None, full_tensorboard_log=False, seed=None,
                 n_cpu_tf_sess=None, device="cuda:0", data_parallel=None, device_norm=None):
        import os
        if data_parallel is None:
            data_parallel = os.environ.get("GRL_DATA_PARALLEL") or None
        if data_parallel not in (None, False, "", "0", "off"):
            raise NotImplementedError("PPO2: data_parallel is not implemented (one replica; use more environments instead)")
        if callable(cliprange) or callable(cliprange_vf):
            raise NotImplementedError("PPO2: a callable cliprange / cliprange_vf is not implemented (the clip ranges are "
                                      "constants of the device plan)")
        self.device_norm = _device_norm_setting(device_norm)
        self.policy, self.policy_kwargs = policy, ({} if policy_kwargs is None else dict(policy_kwargs))
        self.gamma, self.n_steps, self.ent_coef, self.learning_rate = gamma, int(n_steps), ent_coef, learning_rate
        self.vf_coef, self.max_grad_norm, self.lam = vf_coef, max_grad_norm, lam
        self.nminibatches, self.noptepochs = int(nminibatches), int(noptepochs)
        self.cliprange, self.cliprange_vf = cliprange, cliprange_vf
        self.verbose, self.tensorboard_log, self.seed, self.device = verbose, tensorboard_log, seed, device
        self.full_tensorboard_log, self.n_cpu_tf_sess = full_tensorboard_log, n_cpu_tf_sess
        self.num_timesteps, self.n_updates, self.n_batch = 0, 0, None
        self.env = self.observation_space = self.action_space = None
        self.n_envs, self._vec_normalize_env, self.engine = 1, None, None
        self._rng = np.random.RandomState(seed)
        self.ep_info_buf = deque(maxlen=100)
        if env is not None:
            self.set_env(env)
        if _init_setup_model and self.observation_space is not None:
            self.setup_model()

    # ------------------------------------------------------------------ env
    def set_env(self, env):
        if env is not None and not isinstance(env, VecEnv) and not hasattr(env, "num_envs"):
            env = DummyVecEnv([lambda: env])
        if env is not None:
            env = expand_training_env(env)      # GRL_NUM_ENVS: the script's single-factory DummyVecEnv fans out to workers
            if self.observation_space is not None and tuple(env.observation_space.shape) != tuple(self.observation_space.shape):
                raise ValueError("observation space of the new env does not match the model")
            if self.engine is not None and env.num_envs != self.engine.n_envs:
                raise ValueError("PPO2: the env must have the %d sub-environments the model was built for (the rollout's "
                                 "shape is part of the device plan)" % self.engine.n_envs)
            self.observation_space, self.action_space = env.observation_space, env.action_space
            self.n_envs = env.num_envs
            self._vec_normalize_env = unwrap_vec_normalize(env)
        self.env = env

    def get_env(self):
        return self.env

    def get_vec_normalize_env(self):
        return self._vec_normalize_env

    # ------------------------------------------------------------------ model
    def _net_arch(self):
        """(pi widths, vf widths) of policy_kwargs; refuses what the device plan does not build."""
        pol = self.policy
        name = getattr(pol, "__name__", str(pol))
        if isinstance(pol, str):
            if pol != "MlpPolicy":
                raise NotImplementedError("PPO2: policy %r is not implemented (only the actor-critic MlpPolicy)" % pol)
        elif getattr(pol, "feature_extraction", "mlp") == "cnn" or "Lstm" in name or "Cnn" in name:
            raise NotImplementedError("PPO2: policy %s is not implemented (only the actor-critic MlpPolicy: CnnPolicy, "
                                      "MlpLstmPolicy and their relatives are refused)" % name)
        kw = self.policy_kwargs
        act_fun = kw.get("act_fun")
        if act_fun is not None and getattr(act_fun, "__name__", str(act_fun)) != "tanh":
            raise NotImplementedError("PPO2: act_fun %s is not implemented (the towers' activation is tanh)"
                                      % getattr(act_fun, "__name__", act_fun))
        unknown = sorted(set(kw) - {"net_arch", "act_fun", "feature_extraction"})
        if unknown:
            raise NotImplementedError("PPO2: policy_kwargs %s are not implemented" % unknown)
        if kw.get("feature_extraction", "mlp") != "mlp":
            raise NotImplementedError("PPO2: feature_extraction %r is not implemented" % kw["feature_extraction"])
        arch = kw.get("net_arch")
        if arch is None:
            return (64, 64), (64, 64)
        arch = list(arch)
        if len(arch) != 1 or not isinstance(arch[0], dict):
            raise NotImplementedError("PPO2: shared layers in net_arch are not implemented (net_arch must be "
                                      "[dict(vf=[...], pi=[...])], got %r)" % (arch,))
        pi, vf = tuple(int(w) for w in arch[0].get("pi", ())), tuple(int(w) for w in arch[0].get("vf", ()))
        for nm, t in (("pi", pi), ("vf", vf)):
            if not 1 <= len(t) <= _capi.GRL_MAX_LAYERS or any(not 1 <= w <= 1024 for w in t):
                raise NotImplementedError("PPO2: the %s tower needs 1..%d layers of widths 1..1024, got %r"
                                          % (nm, _capi.GRL_MAX_LAYERS, list(t)))
        return pi, vf

    def setup_model(self):
        if not sp.is_box(self.action_space):
            raise NotImplementedError("PPO2: %s action spaces are not implemented (Box only; Discrete / MultiDiscrete are refused)"
                                      % type(self.action_space).__name__)
        if not sp.is_box(self.observation_space) or len(tuple(self.observation_space.shape)) < 1:
            raise ValueError("Box observations expected, got %s" % (self.observation_space,))
        pi, vf = self._net_arch()
        self._obs_dim = int(np.prod(tuple(self.observation_space.shape)))
        self._act_dim = int(np.prod(tuple(self.action_space.shape)))
        self.n_batch = self.n_envs * self.n_steps
        assert self.n_batch % self.nminibatches == 0, "The number of minibatches (`nminibatches`) is not a factor of the " \
            "total number of samples collected per rollout (`n_batch`), some samples won't be used."
        cfg, ppo = _capi.make_ppo_config(self._obs_dim, self._act_dim, n_envs=self.n_envs, n_steps=self.n_steps,
                                         nminibatches=self.nminibatches, pi_layers=pi, vf_layers=vf, gamma=self.gamma, lam=self.lam,
                                         lr=float(_constfn(self.learning_rate)(1.0)), ent_coef=self.ent_coef, vf_coef=self.vf_coef,
                                         max_grad_norm=self.max_grad_norm, cliprange=float(self.cliprange),
                                         cliprange_vf=None if self.cliprange_vf is None else float(self.cliprange_vf),
                                         seed=0 if self.seed is None else int(self.seed), **_normalize_kwargs(self._vec_normalize_env))
        self.engine = self._engine_factory(cfg, ppo, self.device)
        self.engine.set_parameters(init_ppo_parameters(self.engine.table, 0 if self.seed is None else int(self.seed)))

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

    def pretrain(self, dataset, n_epochs=10, learning_rate=1e-4, adam_epsilon=1e-8, val_interval=None):
        raise NotImplementedError("%s: pretrain is not implemented (behaviour cloning runs on SAC models only)" % type(self).__name__)

    # ------------------------------------------------------------------ learn
    def learn(self, total_timesteps, callback=None, log_interval=1, tb_log_name="PPO2", reset_num_timesteps=True):
        if self.env is None:
            raise ValueError("learn() needs an environment")
        total_timesteps = int(total_timesteps)      # (the reference's --timestep arrives as a string)
        if reset_num_timesteps:
            self.num_timesteps = 0
        lr_fn = _constfn(self.learning_rate)
        # a model restored from a checkpoint continues in place (sb/checkpoint.py): the rollout, the update index and the
        # learning-rate schedule's length stand where the saved run left them
        resume = self._take_resume(reset_num_timesteps)
        self._schedule_total = total_timesteps if resume is None else (resume["schedule_total"] or total_timesteps)
        device_norm = self._resolve_device_norm(callback)      # (decided from the callback the USER handed over)
        callback = as_callback(callback)
        callback.init_callback(self)
        # stable-baselines hands callbacks a FileWriter when tensorboard_log is set, None otherwise
        writer = logger.SummaryWriter(self.tensorboard_log, tb_log_name) if self.tensorboard_log else None
        try:
            self._attach_device_norm(device_norm, upload=resume is None)      # restored: the device holds the statistics already
            self._learn_loop(total_timesteps, callback, log_interval, writer, lr_fn, resume)
        finally:
            self._detach_device_norm()
            if writer is not None:
                writer.close()
        return self

    # ------------------------------------------------------------------ VecNormalize observation statistics on the device
    def _resolve_device_norm(self, user_callback):
        from .sac import resolve_device_norm
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

    def _learn_loop(self, total_timesteps, callback, log_interval, writer, lr_fn, resume=None):
        eng, N, T = self.engine, self.n_envs, self.n_steps
        n_updates = total_timesteps // self.n_batch
        saved, finished = None, False
        if resume is None:
            eng.reset_rollout()      # (a run a callback stopped mid-rollout left a slot open)
            obs = np.asarray(self.env.reset(), np.float32)
            dones = np.zeros(N, np.float32)
            updates, sched_updates = range(1, n_updates + 1), n_updates
        else:
            # the restored rollout goes on: the open slot is closed with the restored rewards, the remaining slots are filled,
            # the update index and the schedule's length are the saved run's, and the run ends where num_timesteps has grown by
            # total_timesteps -- at the rollout boundaries the uninterrupted run has (a rollout that would end later is not begun)
            obs, (written, closed, finished), saved = self._resumed_start(resume)
            dones = np.ones(N, np.float32)
            first = (resume["loop"] or {}).get("update", 1)
            left = total_timesteps - (T - written) * N
            updates = range(first, first + (0 if left < 0 else 1 + left // self.n_batch))
            sched_updates = max(1, int(resume["schedule_total"] or total_timesteps) // self.n_batch)
        lp = self._loop = {"update": updates.start, "dones": dones, "infos": (), "ep_infos": [],
                           "values": np.zeros((T, N), np.float32), "rewards": np.zeros((T, N), np.float32)}
        t_first_start = time.time()
        callback.on_training_start(locals(), globals())
        for update in updates:
            t_start = time.time()
            frac = 1.0 - (update - 1.0) / sched_updates
            lr_now = float(lr_fn(frac))
            if saved is None:
                values, rewards, ep_infos = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32), []
                step0, reopened = 0, False
            else:      # the rollout the checkpoint was taken in
                values, rewards, ep_infos = saved["values"].copy(), saved["rewards"].copy(), list(saved["ep_infos"])
                step0, reopened, saved = closed, written == closed + 1, None
            lp.update(update=update, values=values, rewards=rewards, ep_infos=ep_infos, infos=())
            if step0 == 0 and not reopened:
                callback.on_rollout_start()
            # ---- Runner._run: n_steps policy steps; what the update needs stays on the device
            go_on = True
            for step in range(step0, T):
                if reopened:      # written before the save, its rewards and infos taken then: only closing it is left
                    reopened, infos = False, ()
                else:
                    actions, values[step], neglogpacs = eng.step(self._rows(obs, N), dones)
                    clipped_actions = self._clip(actions.reshape((N,) + tuple(self.action_space.shape)))
                    obs, rew, done, infos = self.env.step(clipped_actions)
                    obs, dones = np.asarray(obs, np.float32), np.asarray(done, np.float32).reshape(N)
                    rewards[step] = np.asarray(rew, np.float32).reshape(N)
                    self.num_timesteps += N
                    lp["dones"], lp["infos"] = dones, infos
                    callback.update_locals(locals())
                    if callback.on_step() is False:
                        go_on = False
                        break
                for info in infos:
                    maybe = info.get("episode") if isinstance(info, dict) else None
                    if maybe is not None:
                        ep_infos.append(maybe)
                eng.rewards(rewards[step])
            if not go_on:
                break
            if not finished:      # (a checkpoint taken in on_rollout_end holds the advantages already)
                eng.finish(self._rows(obs, N), dones)      # (device path: the rows serve the next rollout's first step as well)
                callback.on_rollout_end()
            finished = False
            self.ep_info_buf.extend(ep_infos)
            # ---- noptepochs epochs over nminibatches consecutive slices of a fresh permutation each
            eng.set_learning_rate(lr_now)
            want_log = self.verbose >= 1 and log_interval is not None and (update % log_interval == 0 or update == 1)
            returns = eng.fetch("ppo_ret", (N, T)).T if want_log else None
            perm = np.stack([self._rng.permutation(self.n_batch) for _ in range(self.noptepochs)]).astype(np.int32)
            eng.train(perm)
            lp["update"] = update + 1      # (the rollout is empty: the next one belongs to the next update)
            self.n_updates += self.noptepochs * self.nminibatches
            if writer is not None:
                self._write_summary(writer, eng.metrics().mean(axis=0), lr_now)
            if want_log:
                loss_vals = eng.metrics().mean(axis=0)
                t_now = time.time()
                fps = int(self.n_batch / max(t_now - t_start, 1e-9))
                logger.logkv("serial_timesteps", update * T)
                logger.logkv("n_updates", update)
                logger.logkv("total_timesteps", self.num_timesteps)
                logger.logkv("fps", fps)
                logger.logkv("explained_variance", float(explained_variance(values, returns)))
                if len(self.ep_info_buf) > 0 and len(self.ep_info_buf[0]) > 0:
                    logger.logkv("ep_reward_mean", _safe_mean([e["r"] for e in self.ep_info_buf]))
                    logger.logkv("ep_len_mean", _safe_mean([e["l"] for e in self.ep_info_buf]))
                logger.logkv("time_elapsed", t_start - t_first_start)
                for name, val in zip(self.loss_names, loss_vals):
                    logger.logkv(name, float(val))
                logger.dumpkvs()
        callback.on_training_end()

    loss_names = ("policy_loss", "value_loss", "policy_entropy", "approxkl", "clipfrac")

    def _write_summary(self, writer, loss_vals, lr_now):
        tags = ("loss/policy_gradient_loss", "loss/value_function_loss", "loss/entropy_loss", "loss/approximate_kullback-leibler",
                "loss/clip_factor")
        vals = [{"tag": t, "simple_value": float(v)} for t, v in zip(tags, loss_vals)]
        writer.add_summary({"value": vals + [{"tag": "input_info/learning_rate", "simple_value": lr_now}]}, self.num_timesteps)

    # ------------------------------------------------------------------ persistence
    def get_parameter_list(self):
        return self.engine.param_names()

    def get_parameters(self):
        return self.engine.get_parameters()

    def load_parameters(self, load_path_or_dict, exact_match=True):
        params = load_path_or_dict
        if isinstance(params, str):
            _, params = save_util.load_from_zip(params)
        unknown = [k for k in params if k not in set(self.get_parameter_list())]
        if unknown:
            raise RuntimeError("load_parameters: unknown parameter(s) %s" % unknown[:5])
        self.engine.set_parameters(params, exact_match=exact_match)

    _SAVED = ("gamma", "n_steps", "vf_coef", "ent_coef", "max_grad_norm", "lam", "nminibatches", "noptepochs", "cliprange",
              "cliprange_vf", "verbose", "n_cpu_tf_sess", "seed", "policy_kwargs")

    def _save_zip(self, save_path):
        data = {k: getattr(self, k) for k in self._SAVED}
        data["learning_rate"] = float(_constfn(self.learning_rate)(1.0))
        data.update(observation_space=self.observation_space, action_space=self.action_space, policy=self.policy,
                    n_envs=self.n_envs, _vectorize_action=False)
        return save_util.save_to_zip(save_path, data, self.get_parameters())

    @classmethod
    def _load_zip(cls, load_path, env=None, custom_objects=None, **kwargs):
        data, params = save_util.load_from_zip(load_path)
        policy = data.get("policy")
        model = cls(policy=policy if (isinstance(policy, (type, str)) and policy is not None) else "MlpPolicy", env=None,
                    _init_setup_model=False)
        for k, v in data.items():
            if k in cls._SAVED + ("learning_rate",) and (v is not None or k in ("cliprange_vf", "max_grad_norm")):
                setattr(model, k, v)
        model.policy_kwargs = dict(model.policy_kwargs or {})
        for k, v in kwargs.items():
            setattr(model, k, v)
        model._rng = np.random.RandomState(model.seed)
        model.observation_space, model.action_space = data.get("observation_space"), data.get("action_space")
        model.n_envs = int(data.get("n_envs") or 1)
        if env is not None:
            model.set_env(env)
        if model.observation_space is None or model.action_space is None:
            raise ValueError("the zip holds no readable spaces; pass env=")
        if "net_arch" not in model.policy_kwargs:      # the towers as the parameters describe them
            def widths(nm):
                out, l = [], 0
                while "model/%s_fc%d/w:0" % (nm, l) in params:
                    out.append(int(params["model/%s_fc%d/w:0" % (nm, l)].shape[1]))
                    l += 1
                return out
            if (widths("pi"), widths("vf")) != ([64, 64], [64, 64]):
                model.policy_kwargs["net_arch"] = [dict(vf=widths("vf"), pi=widths("pi"))]
        model.setup_model()
        model.load_parameters(params)
        return model
