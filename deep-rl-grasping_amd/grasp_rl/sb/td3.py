"""``TD3`` with the stable-baselines 2.10.1 constructor / learn / predict / save / load surface (td3/td3.py).  The update itself
(replay sampling + normalisation, the policy and twin-critic forward-backward, the smoothed target, both Adams, Polyak) runs in
the HIP engine (grasp_rl.engine.Td3Engine -> libgrl.so, csrc/plan_td3.inl); this file is the host loop of stable-baselines'
``TD3.learn``: act (+ ``action_noise``) -> env.step -> callbacks -> store the raw transition -> every ``train_freq`` steps up to
``gradient_steps`` updates, ONE ``grl_td3_train`` call whose update g is a policy update iff ``(step + g) % policy_delay == 0``.

Vectorised envs with ``num_envs > 1`` are accepted as SAC accepts them (stable-baselines asserts a single env): ``step`` then
counts vectorised steps, ``num_timesteps`` environment steps.  ``action_noise`` is ONE object for all of them, as in SAC's loop:
its draw is added to the [N, A] actions (a noise of shape [A] gives every environment the same draw, one of shape [N, A] a draw
each) and it is ``reset()`` when environment 0 ends an episode -- with N > 1 a noise that carries state between steps
(``OrnsteinUhlenbeckActionNoise``) is therefore reset in the middle of the other environments' episodes.  VecNormalize statistics stay on the host and are pushed to the
engine before an update.  Not implemented, and refused by name: CnnPolicy / LnMlpPolicy / ``layer_norm``, a non-Box action space,
``data_parallel``, ``device_norm=True``, ``save_checkpoint`` / ``load_checkpoint`` and ``pretrain``.
"""
import os
import time
from collections import deque

import numpy as np

from .. import _capi
from ..engine import Td3Engine
from ..init import init_parameters
from . import checkpoint
from . import logger
from . import policies as pol
from . import save_util
from . import spaces as sp
from .base import BaseModel, device_norm_setting
from .callbacks import as_callback

_POLICY_NAMES = {"MlpPolicy": pol.Td3MlpPolicy, "LnMlpPolicy": pol.Td3LnMlpPolicy, "CnnPolicy": pol.Td3CnnPolicy,
                 "LnCnnPolicy": pol.Td3LnCnnPolicy}


class TD3(BaseModel):
    # tests substitute the g++ emulation build here; the product default needs a HIP device
    _engine_factory = staticmethod(lambda cfg, td3, device: Td3Engine(cfg, td3, device=device))

    def __init__(self, policy, env, gamma=0.99, learning_rate=3e-4, buffer_size=50000, learning_starts=100, train_freq=100,
                 gradient_steps=100, batch_size=128, tau=0.005, policy_delay=2, action_noise=None, target_policy_noise=0.2,
                 target_noise_clip=0.5, random_exploration=0.0, verbose=0, tensorboard_log=None, _init_setup_model=True,
                 policy_kwargs=None, full_tensorboard_log=False, seed=None, n_cpu_tf_sess=None, device="cuda:0", device_norm=None,
                 data_parallel=None):
        if isinstance(policy, str):
            if policy not in _POLICY_NAMES:
                raise ValueError("unknown policy %r" % policy)
            policy = _POLICY_NAMES[policy]
        self.policy = policy
        self.policy_kwargs = {} if policy_kwargs is None else dict(policy_kwargs)
        self.gamma, self.learning_rate = gamma, learning_rate
        self.buffer_size, self.learning_starts = int(buffer_size), learning_starts
        self.train_freq, self.gradient_steps, self.batch_size, self.tau = train_freq, gradient_steps, int(batch_size), tau
        self.policy_delay, self.target_policy_noise, self.target_noise_clip = policy_delay, target_policy_noise, target_noise_clip
        self.action_noise, self.random_exploration = action_noise, random_exploration
        self.verbose, self.tensorboard_log = verbose, tensorboard_log
        self.full_tensorboard_log, self.seed, self.n_cpu_tf_sess = full_tensorboard_log, seed, n_cpu_tf_sess
        self.device = device
        if data_parallel is None:
            data_parallel = os.environ.get("GRL_DATA_PARALLEL") or None
        if data_parallel not in (None, False, "", "0", "off"):
            raise NotImplementedError("TD3: data_parallel is not implemented")
        if device_norm_setting(device_norm, unset=False) is True:
            raise NotImplementedError("TD3: device_norm=True is not implemented (the VecNormalize statistics stay on the host)")
        self.num_timesteps = 0
        self.n_updates = 0
        self.env = None
        self.observation_space = self.action_space = None
        self.n_envs = 1
        self._vectorize_action = True
        self._vec_normalize_env = None
        self.engine = None
        self.episode_reward = None
        self._rng = np.random.default_rng(seed)
        if env is not None:
            self.set_env(env)
        if _init_setup_model and self.observation_space is not None:
            self.setup_model()

    # ------------------------------------------------------------------ model
    def setup_model(self):
        if not sp.is_box(self.action_space):
            raise NotImplementedError("TD3: a non-Box action space is not implemented (TD3 needs continuous actions)")
        if getattr(self.policy, "feature_extraction", "mlp") == "cnn" or self.policy_kwargs.get("feature_extraction", "mlp") == "cnn" \
                or "cnn_extractor" in self.policy_kwargs:
            raise NotImplementedError("TD3: CnnPolicy is not implemented (MlpPolicy on vector observations only)")
        if getattr(self.policy, "layer_norm", False):
            raise NotImplementedError("TD3: LnMlpPolicy is not implemented")
        if self.policy_kwargs.get("layer_norm", False):
            raise NotImplementedError("TD3: layer_norm is not implemented")
        unknown = sorted(set(self.policy_kwargs) - {"layers", "layer_norm", "feature_extraction"})
        if unknown:
            raise NotImplementedError("TD3: policy_kwargs %s are not implemented" % unknown)
        obs_shape = tuple(self.observation_space.shape)
        if len(obs_shape) != 1:
            raise ValueError("MlpPolicy expects vector observations, got shape %s" % (obs_shape,))
        vn = self._vec_normalize_env
        kw = {} if vn is None else dict(clip_obs=vn.clip_obs, clip_reward=vn.clip_reward, norm_eps=vn.epsilon)
        cfg, td3 = _capi.make_td3_config(obs_shape[0], int(np.prod(self.action_space.shape)), layers=tuple(self.policy_kwargs.get("layers", (64, 64))),
                                         batch_size=self.batch_size, act_batch=max(1, self.n_envs), replay_capacity=self.buffer_size,
                                         normalize=0 if vn is None else _capi.norm_mode(vn), gamma=self.gamma, lr=self._learning_rate_value(),
                                         tau=self.tau, policy_delay=int(self.policy_delay), target_policy_noise=float(self.target_policy_noise),
                                         target_noise_clip=float(self.target_noise_clip), seed=0 if self.seed is None else int(self.seed), **kw)
        if self.seed is not None and hasattr(self.action_space, "seed"):     # BaseRLModel.set_random_seed: action_space.seed(seed)
            self.action_space.seed(int(self.seed))
        self._norm_stamp = None         # a new engine starts with zero statistics
        self.engine = self._engine_factory(cfg, td3, self.device)
        self.engine.set_parameters(init_parameters(self.engine.table, seed=0 if self.seed is None else int(self.seed)))

    def set_env(self, env):
        super().set_env(env)
        if env is not None:
            self._norm_stamp = None     # a new wrapper: its statistics must reach the device whatever their counts are

    def _sync_norm_stats(self):
        """VecNormalize statistics move on the env side every step and are read at sample time with their current values:
        pushed to the engine before an update, when they have moved."""
        vn = self._vec_normalize_env
        if vn is None or not self.engine.cfg.normalize:
            return
        stamp = (id(vn.obs_rms), float(vn.obs_rms.count), id(vn.ret_rms), float(vn.ret_rms.count),
                 float(np.sum(vn.obs_rms.mean)), float(np.sum(vn.obs_rms.var)), float(np.sum(vn.ret_rms.var)))
        if stamp == self._norm_stamp:
            return
        self._norm_stamp = stamp
        self.engine.set_obs_stats(vn.obs_rms.mean, vn.obs_rms.var, float(vn.ret_rms.var))   # asynchronous, stream-ordered

    # ------------------------------------------------------------------ acting
    def _act(self, obs):
        obs = np.asarray(obs, np.float32).reshape(len(obs), -1)
        out = np.empty((len(obs), int(np.prod(self.action_space.shape))), np.float32)
        cap = self.engine.cfg.act_batch
        for k0 in range(0, len(obs), cap):
            out[k0:k0 + cap] = self.engine.act(obs[k0:k0 + cap])
        return out

    def _unscale(self, a):
        low, high = np.asarray(self.action_space.low, np.float32), np.asarray(self.action_space.high, np.float32)
        return low + 0.5 * (a + 1.0) * (high - low)

    def _scale(self, a):
        low, high = np.asarray(self.action_space.low, np.float32), np.asarray(self.action_space.high, np.float32)
        return 2.0 * (a - low) / (high - low) - 1.0

    def predict(self, observation, state=None, mask=None, deterministic=True):
        observation = np.asarray(observation)
        single = observation.shape == tuple(self.observation_space.shape)
        act = self._act(observation.reshape((-1,) + tuple(self.observation_space.shape)))
        if self.action_noise is not None and not deterministic:
            act = np.clip(act + self.action_noise(), -1, 1)
        act = self._unscale(act).reshape((-1,) + tuple(self.action_space.shape))
        act = np.clip(act, self.action_space.low, self.action_space.high)
        return (act[0] if single else act), None

    # ------------------------------------------------------------------ learn
    def learn(self, total_timesteps, callback=None, log_interval=4, tb_log_name="TD3", reset_num_timesteps=True, replay_wrapper=None):
        total_timesteps, _ = self._begin_learn(total_timesteps, reset_num_timesteps)
        callback = as_callback(callback)
        callback.init_callback(self)
        eng, vn, N = self.engine, self._vec_normalize_env, self.n_envs
        episode_rewards, episode_successes, ep_info_buf = [0.0], [], deque(maxlen=100)
        self.episode_reward = np.zeros((N,))
        n_episodes, infos_values = 0, None
        start = time.time()
        writer = logger.SummaryWriter(self.tensorboard_log, tb_log_name) if self.tensorboard_log else None
        if self.action_noise is not None:
            self.action_noise.reset()
        obs = self.env.reset()
        obs_ = vn.get_original_obs() if vn is not None else obs
        callback.on_training_start(locals(), globals())
        callback.on_rollout_start()
        step = 0                # vectorised env steps taken (stable-baselines' `step`, one environment)
        end = self.num_timesteps + total_timesteps
        try:
            while self.num_timesteps < end:
                # uniform actions before learning_starts and, afterwards, with probability random_exploration
                if self.num_timesteps < self.learning_starts or self._rng.random() < self.random_exploration:
                    unscaled_action = np.stack([np.asarray(self.action_space.sample(), np.float32) for _ in range(N)])
                    action = self._scale(unscaled_action)
                else:
                    action = self._act(obs)
                    if self.action_noise is not None:
                        action = np.clip(action + self.action_noise(), -1, 1)
                    unscaled_action = self._unscale(action)
                new_obs, reward, done, info = self.env.step(unscaled_action.reshape((N,) + tuple(self.action_space.shape)))
                self.num_timesteps += N
                callback.update_locals(locals())
                if callback.on_step() is False:
                    break
                if vn is not None:
                    new_obs_, reward_ = vn.get_original_obs(), vn.get_original_reward()
                else:
                    new_obs_, reward_ = new_obs, reward
                # an auto-reset env returns the first observation of the next episode: the replay row keeps the terminal one
                next_store = np.array(new_obs_, np.float32, copy=True)
                for i in range(N):
                    if done[i] and isinstance(info[i], dict) and "terminal_observation" in info[i]:
                        next_store[i] = info[i]["terminal_observation"]
                eng.replay_add(np.asarray(obs_, np.float32), action.reshape(N, -1), np.asarray(reward_, np.float32), next_store,
                               np.asarray(done, np.float32))
                obs, obs_ = new_obs, new_obs_
                if step % self.train_freq == 0:
                    callback.on_rollout_end()
                    # stable-baselines breaks out of its gradient_steps loop while the replay cannot fill a batch or learning has
                    # not started: neither changes inside the loop, so it runs all of its updates or none
                    k = int(self.gradient_steps)
                    if k > 0 and eng.replay_size() >= self.batch_size and self.num_timesteps >= self.learning_starts:
                        self._sync_norm_stats()
                        if callable(self.learning_rate):    # frac = 1 - step / total (step: the environment steps before this one)
                            eng.set_learning_rate(self.learning_rate(1.0 - step * N / max(1, self._schedule_total)))
                        for g0 in range(0, k, _capi.TD3_MAX_UPDATES):
                            eng.train(min(_capi.TD3_MAX_UPDATES, k - g0), first_step=step + g0)
                        self.n_updates += k
                    callback.on_rollout_start()
                step += 1
                for i in range(N):
                    maybe = info[i].get("episode") if isinstance(info[i], dict) else None
                    if maybe is not None:
                        ep_info_buf.append(maybe)
                    if isinstance(info[i], dict) and info[i].get("is_success") is not None and done[i]:
                        episode_successes.append(float(info[i]["is_success"]))
                self.episode_reward += np.asarray(reward_, np.float64).reshape(N)
                episode_rewards[-1] += float(np.asarray(reward_).reshape(N)[0])
                if done[0]:
                    if self.action_noise is not None:      # (one object for all N environments: module docstring)
                        self.action_noise.reset()
                    episode_rewards.append(0.0)
                    n_episodes += 1
                    if self.verbose >= 1 and log_interval is not None and n_episodes % log_interval == 0:
                        logger.logkv("episodes", n_episodes)
                        logger.logkv("mean 100 episode reward", round(float(np.mean(episode_rewards[-101:-1])), 1))
                        if ep_info_buf:
                            logger.logkv("ep_rewmean", float(np.mean([e["r"] for e in ep_info_buf])))
                            logger.logkv("eplenmean", float(np.mean([e["l"] for e in ep_info_buf])))
                        logger.logkv("n_updates", self.n_updates)
                        logger.logkv("current_lr", self._learning_rate_value())
                        logger.logkv("fps", int(self.num_timesteps / (time.time() - start + 1e-9)))
                        logger.logkv("time_elapsed", int(time.time() - start))
                        if episode_successes:
                            logger.logkv("success rate", float(np.mean(episode_successes[-100:])))
                        if self.n_updates > 0:
                            infos_values = eng.metrics().mean(axis=0)
                            for name, v in zip(eng.METRIC_NAMES[:5], infos_values):
                                logger.logkv(name, float(v))
                        logger.logkv("total timesteps", self.num_timesteps)
                        logger.dumpkvs()
            callback.on_training_end()
        finally:
            if writer is not None:
                writer.close()
        return self

    # ------------------------------------------------------------------ parameters / persistence
    def _data(self):
        return {
            "learning_rate": self._learning_rate_value(), "buffer_size": self.buffer_size, "learning_starts": self.learning_starts,
            "train_freq": self.train_freq, "gradient_steps": self.gradient_steps, "batch_size": self.batch_size, "tau": self.tau,
            "policy_delay": self.policy_delay, "target_policy_noise": self.target_policy_noise, "target_noise_clip": self.target_noise_clip,
            "gamma": self.gamma, "verbose": self.verbose, "observation_space": self.observation_space, "action_space": self.action_space,
            "policy": self.policy, "n_envs": self.n_envs, "n_cpu_tf_sess": self.n_cpu_tf_sess, "seed": self.seed,
            "action_noise": self.action_noise, "random_exploration": self.random_exploration,
            "_vectorize_action": self._vectorize_action, "policy_kwargs": self.policy_kwargs,
        }

    def _save_zip(self, save_path):
        return save_util.save_to_zip(save_path, self._data(), self.get_parameters())

    def save(self, save_path, cloudpickle=False):
        if checkpoint.enabled():
            raise NotImplementedError("TD3: save_checkpoint is not implemented (GRL_CHECKPOINT_STATE=1 asks save() for one)")
        return self._save_zip(save_path)

    @classmethod
    def load(cls, load_path, env=None, custom_objects=None, **kwargs):
        return cls._load_zip(load_path, env=env, custom_objects=custom_objects, **kwargs)

    def save_checkpoint(self, path, include_replay=True):
        raise NotImplementedError("TD3: save_checkpoint is not implemented")

    @classmethod
    def load_checkpoint(cls, path, env=None, **kwargs):
        raise NotImplementedError("TD3: load_checkpoint is not implemented")

    @classmethod
    def _load_zip(cls, load_path, env=None, custom_objects=None, **kwargs):
        data, params = save_util.load_from_zip(load_path)
        if "policy_kwargs" in kwargs and kwargs["policy_kwargs"] != data.get("policy_kwargs"):
            raise ValueError("the specified policy kwargs do not equal the stored policy kwargs")
        policy = data.get("policy")
        if policy is None or not isinstance(policy, type):
            policy = pol.Td3MlpPolicy
        if not isinstance(data.get("policy_kwargs"), dict):
            data["policy_kwargs"] = pol.infer_sac_policy_kwargs(params)[1]      # layers = widths of model/pi/fc<l>/kernel:0
        model = cls(policy=policy, env=None, _init_setup_model=False)
        for k in ("gamma", "buffer_size", "learning_starts", "train_freq", "gradient_steps", "batch_size", "tau", "policy_delay",
                  "target_policy_noise", "target_noise_clip", "verbose", "n_envs", "seed", "random_exploration", "policy_kwargs",
                  "action_noise"):
            if k in data and data[k] is not None:
                setattr(model, k, data[k])
        if isinstance(data.get("learning_rate"), (int, float)):
            model.learning_rate = float(data["learning_rate"])
        return model._finish_load(data, params, env, kwargs)
