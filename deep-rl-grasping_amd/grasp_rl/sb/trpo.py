"""``TRPO`` with the constructor / learn / predict / save / load surface the reference uses
(/root/reference/manipulation_main/training/sb_helper.py:129-136 ``sb.TRPO(MlpPolicy, env, verbose=2, gamma=...,
timesteps_per_batch=config['TRPO']['max_iters'], vf_stepsize=config['TRPO']['step_size'], tensorboard_log=...)``; loader at
train_stable_baselines.py:95-96).

Everything that touches a tensor runs in the HIP engine (``TrpoEngine``; csrc/plan_trpo.inl, csrc/trpo_kernels.h): the policy
step writes observation, action and value straight into the rollout on the device; GAE, the advantage standardisation, the
gradient, conjugate gradient on the Fisher-vector product, the line search and the Adam fit of the value tower read it there.
This file is the host loop of stable-baselines 2.10.1 ``TRPO.learn`` / ``traj_segment_generator``: the env steps of ONE
environment (actions clipped to the space for the env only; after a ``done`` the generator's own ``env.reset()``), the callback
protocol, ``vf_iters`` permutations per batch from the model's seeded generator, episode statistics and the logger.
``num_timesteps`` grows by ``timesteps_per_batch`` after every batch, as in stable-baselines.

One deliberate deviation: stable-baselines draws the first action of a batch BEFORE the update of the previous one and
re-evaluates only its value afterwards.  Here ``finish`` evaluates V(last observation) and the next ``step`` draws from the
updated policy.

Scope: the actor-critic ``MlpPolicy`` (two tanh towers, ``net_arch=[dict(vf=[...], pi=[...])]``) on ``Box`` actions, observations
of any rank flattened in C order and not divided by 255, one environment (GRL_NUM_ENVS does not fan a TRPO env out).  The GAIL
keywords and data parallelism are not defined for TRPO; GAIL is a class of its own (gail.py) over the two hooks of ``_learn_loop``.  Everything else says what it refuses.  ``save_checkpoint`` / ``load_checkpoint`` -- or
GRL_CHECKPOINT_STATE=1 behind ``save`` / ``load`` -- keep the full training state next to the zip, and
``learn(n, reset_num_timesteps=False)`` on a restored model continues the batch that was in progress.  The policy this class
accepts, acting, the frame of ``learn`` and the host half of a checkpoint are ``OnPolicyModel`` (on_policy.py), shared with ``PPO2``.

VecNormalize works on the host by default; ``device_norm=True`` (GRL_DEVICE_NORM=1 / auto; unset means off) keeps its observation
statistics on the device while ``learn`` runs (``OnPolicyModel``, the same code as for ``PPO2(device_norm=...)``): one
``engine.observe`` per env step and per reset, ``step`` / ``finish`` on the rows it normalised, rewards on the host.
"""
import os
import time
from collections import OrderedDict, deque

import numpy as np

from .. import _capi
from ..engine import TrpoEngine
from ..init import init_ppo_parameters
from . import logger
from . import save_util
from .base import device_norm_setting
from .on_policy import OnPolicyModel, _normalize_kwargs, _safe_mean, explained_variance

VF_BATCH = 128      # trpo_mpi.py: dataset.iterbatches(..., batch_size=128, include_final_partial_batch=False)


class TRPO(OnPolicyModel):
    _engine_factory = staticmethod(lambda cfg, trpo, device: TrpoEngine(cfg, trpo, device=device))

    def __init__(self, policy, env, gamma=0.99, timesteps_per_batch=1024, max_kl=0.01, cg_iters=10, lam=0.98, entcoeff=0.0,
                 cg_damping=1e-2, vf_stepsize=3e-4, vf_iters=3, verbose=0, tensorboard_log=None, _init_setup_model=True,
                 policy_kwargs=None, full_tensorboard_log=False, seed=None, n_cpu_tf_sess=1, device="cuda:0", device_norm=None,
                 **gail):
        if policy is None:
            raise NotImplementedError("TRPO: policy None is not implemented (only the actor-critic MlpPolicy)")
        if gail:
            known = {"using_gail", "reward_giver", "expert_dataset", "g_step", "d_step", "d_stepsize", "hidden_size_adversary",
                     "adversary_entcoeff"}
            unknown = sorted(set(gail) - known)
            if unknown:
                raise TypeError("TRPO: unexpected keyword arguments %s" % unknown)
            raise NotImplementedError("TRPO: the GAIL arguments %s are not implemented (no adversary on the device)" % sorted(gail))
        if os.environ.get("GRL_DATA_PARALLEL") not in (None, "", "0", "off"):
            raise NotImplementedError("TRPO: data_parallel is not implemented (one replica, one environment)")
        self.device_norm = device_norm_setting(device_norm, unset=False)
        self.policy, self.policy_kwargs = policy, ({} if policy_kwargs is None else dict(policy_kwargs))
        self.gamma, self.timesteps_per_batch, self.max_kl, self.cg_iters = gamma, int(timesteps_per_batch), max_kl, int(cg_iters)
        self.lam, self.entcoeff, self.cg_damping, self.vf_stepsize, self.vf_iters = lam, entcoeff, cg_damping, vf_stepsize, int(vf_iters)
        self.verbose, self.tensorboard_log, self.seed, self.device = verbose, tensorboard_log, seed, device
        self.full_tensorboard_log, self.n_cpu_tf_sess = full_tensorboard_log, n_cpu_tf_sess
        # the GAIL fields of stable-baselines 2.10.1, at their defaults (written into the zip)
        self.using_gail, self.expert_dataset, self.g_step, self.d_step, self.d_stepsize = False, None, 1, 1, 3e-4
        self.hidden_size_adversary, self.adversary_entcoeff = 100, 1e-3
        self.num_timesteps, self.n_batch = 0, None
        self.env = self.observation_space = self.action_space = None
        self.n_envs, self._vec_normalize_env, self.engine = 1, None, None
        self._rng = np.random.RandomState(seed)
        # oldpi/* of a zip: before the first update a copy of model/* (or what a loaded zip carried); afterwards the snapshot the
        # device took at the start of the last update ("trpo_theta_old"), fetched when save() asks for it
        self._oldpi, self._updated = None, False
        self.ep_info_buf = deque(maxlen=100)
        self.len_buffer, self.rew_buffer = deque(maxlen=40), deque(maxlen=40)
        self.episodes_so_far = 0
        if env is not None:
            self.set_env(env)
        if _init_setup_model and self.observation_space is not None:
            self.setup_model()

    # ------------------------------------------------------------------ env
    def _training_env(self, env):      # (GRL_NUM_ENVS does not fan a TRPO env out)
        if env.num_envs != 1:
            raise ValueError("Error: the model requires a non vectorized environment or a single vectorized environment.")
        return env

    # ------------------------------------------------------------------ model
    def setup_model(self):
        self._check_spaces()
        if not 1 <= self.timesteps_per_batch <= 65536:
            raise NotImplementedError("TRPO: timesteps_per_batch must be 1..65536, got %d" % self.timesteps_per_batch)
        if not 1 <= self.cg_iters <= 64:
            raise NotImplementedError("TRPO: cg_iters must be 1..64, got %d" % self.cg_iters)
        if not 0 <= self.vf_iters <= _capi.PPO_MAX_EPOCHS:
            raise NotImplementedError("TRPO: vf_iters must be 0..%d, got %d" % (_capi.PPO_MAX_EPOCHS, self.vf_iters))
        pi, vf = self._net_arch()
        self.n_batch = self.timesteps_per_batch
        cfg, trpo = _capi.make_trpo_config(self._obs_dim, self._act_dim, timesteps_per_batch=self.timesteps_per_batch, pi_layers=pi,
                                           vf_layers=vf, gamma=self.gamma, lam=self.lam, max_kl=self.max_kl, cg_iters=self.cg_iters,
                                           cg_damping=self.cg_damping, entcoeff=self.entcoeff, vf_stepsize=float(self.vf_stepsize),
                                           vf_batch=VF_BATCH, seed=0 if self.seed is None else int(self.seed),
                                           **_normalize_kwargs(self._vec_normalize_env))
        self.engine = self._engine_factory(cfg, trpo, self.device)
        self.engine.set_parameters(init_ppo_parameters(self.engine.table, 0 if self.seed is None else int(self.seed)))

    @property
    def n_vf_minibatches(self):
        """Value minibatches of one iteration: floor(T / 128) per vf_iter, the partial batch at the end dropped."""
        return self.vf_iters * (self.timesteps_per_batch // VF_BATCH)

    # ------------------------------------------------------------------ learn
    def learn(self, total_timesteps, callback=None, log_interval=100, tb_log_name="TRPO", reset_num_timesteps=True):
        return self._learn(total_timesteps, callback, log_interval, tb_log_name, reset_num_timesteps)

    # ------------------------------------------------------------------ checkpoint / resume (sb/checkpoint.py)
    def _host_extra(self):
        """What this class carries beside the shared host state: the episode statistics of the log line and oldpi/* of the zip (the
        device's snapshot lives in scratch a checkpoint does not hold, so it is fetched here)."""
        old = self._oldpi
        if self._updated:
            snap, params = self.engine.fetch("trpo_theta_old"), self.get_parameters()
            old = OrderedDict((n, snap[off:off + numel].reshape(shape).copy() if trainable else params[n])
                              for n, off, numel, shape, trainable in self.engine.table)
        return {"len_buffer": list(self.len_buffer), "rew_buffer": list(self.rew_buffer), "episodes_so_far": self.episodes_so_far,
                "oldpi": old}

    def _set_host_extra(self, extra):
        self.len_buffer, self.rew_buffer = deque(extra["len_buffer"], maxlen=40), deque(extra["rew_buffer"], maxlen=40)
        self.episodes_so_far = extra["episodes_so_far"]
        self._oldpi, self._updated = extra["oldpi"], False

    # the two places where GAIL (gail.py) differs from TRPO inside an iteration; nothing happens here
    def _before_finish(self, eng, episode_start, ep_rets):
        """The T slots are closed, GAE is not formed yet."""

    def _after_update(self, eng, iters_so_far):
        """The policy step and the value fit of iteration ``iters_so_far`` (counted from 0) are enqueued."""

    def _learn_loop(self, total_timesteps, callback, log_interval, writer, resume=None):
        eng, T = self.engine, self.timesteps_per_batch
        saved, finished, written, closed = None, False, 0, 0
        episode_start = np.ones(1, np.float32)
        cur_ep_ret, cur_ep_len = 0.0, 0
        timesteps_so_far, iters_so_far, t_start = 0, 0, time.time()
        if resume is None:
            eng.reset_rollout()      # (a run a callback stopped mid-batch left a slot open)
            obs = np.asarray(self.env.reset(), np.float32)
            end = total_timesteps
        else:
            # the restored batch goes on (on_policy.py: _resumed_start): the generator's counters are the saved run's, and the run
            # ends where its timesteps_so_far has grown by total_timesteps; episode_start is 1 at the seam
            obs, (written, closed, finished), saved = self._resumed_start(resume)
            st = resume["loop"] or {}
            timesteps_so_far, iters_so_far = st.get("timesteps_so_far", 0), st.get("iters_so_far", 0)
            if saved is not None and written == closed + 1:      # (no open slot: the seam cuts the episode, the counters start over)
                cur_ep_ret, cur_ep_len = saved["cur_ep_ret"], saved["cur_ep_len"]
            end = timesteps_so_far + total_timesteps
        lp = self._loop = {"update": iters_so_far + 1, "dones": episode_start, "infos": (), "ep_infos": [], "done": False,
                           "values": np.zeros(T, np.float32), "rewards": np.zeros(T, np.float32), "ep_rets": [], "ep_lens": [],
                           "cur_ep_ret": cur_ep_ret, "cur_ep_len": cur_ep_len, "timesteps_so_far": timesteps_so_far,
                           "iters_so_far": iters_so_far}
        callback.on_training_start(locals(), globals())
        while timesteps_so_far < end:
            if saved is None:
                vpreds, rewards, ep_rets, ep_lens, ep_infos = np.zeros(T, np.float32), np.zeros(T, np.float32), [], [], []
                step0, reopened = 0, False
            else:      # the batch the checkpoint was taken in
                vpreds, rewards, ep_infos = saved["values"].copy(), saved["rewards"].copy(), list(saved["ep_infos"])
                ep_rets, ep_lens, done = list(saved["ep_rets"]), list(saved["ep_lens"]), saved["done"]
                step0, reopened, saved = closed, written == closed + 1, None
            lp.update(values=vpreds, rewards=rewards, ep_infos=ep_infos, ep_rets=ep_rets, ep_lens=ep_lens, infos=())
            if step0 == 0 and not reopened:
                callback.on_rollout_start()
            # ---- traj_segment_generator: T policy steps of the one environment; what the update needs stays on the device
            go_on = True
            for step in range(step0, T):
                if reopened:      # written before the save, its reward, flag and infos taken then: only closing it is left
                    infos = ()
                else:
                    actions, vpred, _ = eng.step(self._rows(obs, 1), episode_start)
                    vpreds[step] = vpred[0]
                    clipped_actions = self._clip(actions.reshape((1,) + tuple(self.action_space.shape)))
                    obs, rew, done, infos = self.env.step(clipped_actions)
                    obs = np.asarray(obs, np.float32)
                    rewards[step] = float(np.asarray(rew).reshape(-1)[0])
                    lp.update(done=bool(np.asarray(done).reshape(-1)[0]), infos=infos, cur_ep_ret=cur_ep_ret, cur_ep_len=cur_ep_len)
                    callback.update_locals(locals())
                    if callback.on_step() is False:
                        go_on = False
                        break
                eng.rewards(rewards[step:step + 1])
                cur_ep_ret += float(rewards[step])
                cur_ep_len += 1
                done = bool(np.asarray(done).reshape(-1)[0])
                episode_start[0] = 1.0 if done else 0.0
                for info in infos:
                    maybe = info.get("episode") if isinstance(info, dict) else None
                    if maybe is not None:
                        ep_infos.append(maybe)
                if done:
                    ep_rets.append(cur_ep_ret)
                    ep_lens.append(cur_ep_len)
                    cur_ep_ret, cur_ep_len = 0.0, 0
                    obs = np.asarray(self.env.reset(), np.float32)
                elif reopened:      # the seam cuts the episode the saved run was in: the fresh environment starts one
                    episode_start[0], cur_ep_ret, cur_ep_len = 1.0, 0.0, 0
                reopened = False
            if not go_on:
                break
            lp.update(cur_ep_ret=cur_ep_ret, cur_ep_len=cur_ep_len)
            if not finished:      # (a checkpoint taken in on_rollout_end holds the advantages already)
                self._before_finish(eng, episode_start, ep_rets)
                eng.finish(self._rows(obs, 1), episode_start)      # nextvpred = V(obs_T) * (1 - episode_start_T), GAE, tdlamret
                callback.on_rollout_end()
            finished = False
            self.ep_info_buf.extend(ep_infos)
            want_log = self.verbose >= 1
            tdlamret = eng.fetch("ppo_ret", (T,)) if want_log else None
            vf_perm = (np.stack([self._rng.permutation(T) for _ in range(self.vf_iters)]).astype(np.int32)
                       if self.vf_iters > 0 and T >= VF_BATCH else None)
            eng.update(vf_perm)
            self._updated = True
            self._after_update(eng, iters_so_far)
            timesteps_so_far += T
            self.num_timesteps += T
            iters_so_far += 1
            lp.update(update=iters_so_far + 1, timesteps_so_far=timesteps_so_far, iters_so_far=iters_so_far)
            self.episodes_so_far += len(ep_lens)
            self.len_buffer.extend(ep_lens)
            self.rew_buffer.extend(ep_rets)
            if writer is not None or want_log:
                m = eng.metrics()
                self.last_metrics = m
            if writer is not None:
                tags = (("loss/policy_gradient_loss", "optimgain"), ("loss/approximate_kullback-leibler", "meankl"),
                        ("loss/entropy_loss", "entbonus"), ("loss/surrogate_gain", "surrgain"), ("loss/policy_entropy", "meanent"))
                writer.add_summary({"value": [{"tag": t, "simple_value": m[k]} for t, k in tags]}, self.num_timesteps)
            if want_log:
                logger.logkv("explained_variance_tdlam_before", float(explained_variance(vpreds, tdlamret)))
                for name, key in (("optimgain", "optimgain"), ("meankl", "meankl"), ("entloss", "entbonus"), ("surrgain", "surrgain"),
                                  ("entropy", "meanent")):
                    logger.logkv(name, m[key])
                if len(self.len_buffer) > 0:
                    logger.logkv("EpLenMean", _safe_mean(self.len_buffer))
                    logger.logkv("EpRewMean", _safe_mean(self.rew_buffer))
                logger.logkv("EpThisIter", len(ep_lens))
                logger.logkv("EpisodesSoFar", self.episodes_so_far)
                logger.logkv("TimestepsSoFar", self.num_timesteps)
                logger.logkv("TimeElapsed", time.time() - t_start)
                logger.dumpkvs()
        callback.on_training_end()

    # ------------------------------------------------------------------ persistence
    _SAVED = ("gamma", "timesteps_per_batch", "max_kl", "cg_iters", "lam", "entcoeff", "cg_damping", "vf_stepsize", "vf_iters",
              "hidden_size_adversary", "adversary_entcoeff", "expert_dataset", "g_step", "d_step", "d_stepsize", "using_gail", "verbose",
              "n_cpu_tf_sess", "seed", "policy_kwargs")

    def load_parameters(self, load_path_or_dict, exact_match=True):
        params = load_path_or_dict
        if isinstance(params, str):
            _, params = save_util.load_from_zip(params)
        if isinstance(params, dict):      # a zip carries oldpi/* behind model/*: the engine keeps the old policy only for the length of an update
            params = OrderedDict((n, a) for n, a in params.items() if not n.startswith("oldpi/"))
        super().load_parameters(params, exact_match=exact_match)

    def _save_zip(self, save_path):
        data = {k: getattr(self, k) for k in self._SAVED}
        data.update(observation_space=self.observation_space, action_space=self.action_space, policy=self.policy, n_envs=self.n_envs,
                    _vectorize_action=False)
        params = OrderedDict(self.get_parameters())
        old = self._oldpi if self._oldpi is not None else params      # before the first update oldpi is a copy of pi
        if self._updated:      # every trainable variable as the last update found it; model/q never moves
            snap = self.engine.fetch("trpo_theta_old")
            old = OrderedDict((n, snap[off:off + numel].reshape(shape) if trainable else params[n])
                              for n, off, numel, shape, trainable in self.engine.table)
        for n in list(params):
            params["oldpi/" + n[len("model/"):]] = np.asarray(old[n]).copy()
        return save_util.save_to_zip(save_path, data, params)

    @classmethod
    def _load_zip(cls, load_path, env=None, custom_objects=None, **kwargs):
        data, params = save_util.load_from_zip(load_path)
        policy = data.get("policy")
        model = cls(policy=policy if (isinstance(policy, (type, str)) and policy is not None) else "MlpPolicy", env=None,
                    _init_setup_model=False)
        for k, v in data.items():
            if k in cls._SAVED and (v is not None or k in ("expert_dataset", "seed")):
                setattr(model, k, v)
        model._finish_load(data, params, env, kwargs)
        old = OrderedDict(("model/" + n[len("oldpi/"):], a) for n, a in params.items() if n.startswith("oldpi/"))
        model._oldpi = old if old else None
        return model
