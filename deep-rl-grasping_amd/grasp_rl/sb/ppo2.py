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
in progress (``_resumed_start``: the open slot, the seam).  What this class shares with ``TRPO`` -- the policy it accepts, acting,
the frame of ``learn``, the device-side statistics and the host half of a checkpoint -- is ``OnPolicyModel`` (on_policy.py).

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
from .base import device_norm_setting
from .on_policy import OnPolicyModel, _normalize_kwargs, _safe_mean, explained_variance


def _constfn(v):
    return v if callable(v) else (lambda _frac: float(v))


class PPO2(OnPolicyModel):
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
        self.device_norm = device_norm_setting(device_norm, unset=False)
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
    def _check_fits_engine(self, env):
        if env.num_envs != self.engine.n_envs:
            raise ValueError("PPO2: the env must have the %d sub-environments the model was built for (the rollout's "
                             "shape is part of the device plan)" % self.engine.n_envs)

    # ------------------------------------------------------------------ model
    def setup_model(self):
        self._check_spaces()
        pi, vf = self._net_arch()
        self.n_batch = self.n_envs * self.n_steps
        assert self.n_batch % self.nminibatches == 0, "The number of minibatches (`nminibatches`) is not a factor of the " \
            "total number of samples collected per rollout (`n_batch`), some samples won't be used."
        cfg, ppo = _capi.make_ppo_config(self._obs_dim, self._act_dim, n_envs=self.n_envs, n_steps=self.n_steps,
                                         nminibatches=self.nminibatches, pi_layers=pi, vf_layers=vf, gamma=self.gamma, lam=self.lam,
                                         lr=self._learning_rate_value(), ent_coef=self.ent_coef, vf_coef=self.vf_coef,
                                         max_grad_norm=self.max_grad_norm, cliprange=float(self.cliprange),
                                         cliprange_vf=None if self.cliprange_vf is None else float(self.cliprange_vf),
                                         seed=0 if self.seed is None else int(self.seed), **_normalize_kwargs(self._vec_normalize_env))
        self.engine = self._engine_factory(cfg, ppo, self.device)
        self.engine.set_parameters(init_ppo_parameters(self.engine.table, 0 if self.seed is None else int(self.seed)))

    # ------------------------------------------------------------------ learn
    def learn(self, total_timesteps, callback=None, log_interval=1, tb_log_name="PPO2", reset_num_timesteps=True):
        return self._learn(total_timesteps, callback, log_interval, tb_log_name, reset_num_timesteps)

    def _learn_loop(self, total_timesteps, callback, log_interval, writer, resume=None):
        eng, N, T = self.engine, self.n_envs, self.n_steps
        lr_fn = _constfn(self.learning_rate)
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
    _SAVED = ("gamma", "n_steps", "vf_coef", "ent_coef", "max_grad_norm", "lam", "nminibatches", "noptepochs", "cliprange",
              "cliprange_vf", "verbose", "n_cpu_tf_sess", "seed", "policy_kwargs")

    def _save_zip(self, save_path):
        data = {k: getattr(self, k) for k in self._SAVED}
        data["learning_rate"] = self._learning_rate_value()
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
        return model._finish_load(data, params, env, kwargs)

    def _before_setup(self, data, params):
        if self.env is None:      # (the rollout's shape is part of the plan: built for as many environments as the saved model had)
            self.n_envs = int(data.get("n_envs") or 1)
        super()._before_setup(data, params)
