"""``DQN`` and ``BDQ`` with the constructor / learn / predict / save / load surface the reference uses
(/root/reference/manipulation_main/training/sb_helper.py:159-165 ``sb.DQN(DQNMlpPolicy, env, verbose,
gamma, batch_size, prioritized_replay, tensorboard_log)``; :202-226 ``sb.BDQ(MlpActPolicy, env, ...,
policy_kwargs={'layers': [[common],[branch],[value]]}, epsilon_greedy, exploration_fraction,
exploration_final_eps, num_actions_pad, learning_starts, target_network_update_freq,
prioritized_replay)``; loaders at train_stable_baselines.py:101-104).

The network update (dueling towers, double-Q target, Huber / squared TD loss, per-variable gradient
clipping, Adam, hard target copy) runs in the HIP engine (``QEngine``); this file is the host loop:
epsilon-greedy exploration, replay bookkeeping and -- when ``prioritized_replay=True`` -- the
proportional prioritised sampler (sum-tree on the host, as stable-baselines does; a device-side tree
is SURVEY.md 8f row 4).  DQN follows stock stable-baselines 2.10.1; BDQ follows the decisions
documented in SURVEY.md A.6 / oracle/dqn.py (the fork's source is unavailable: parity unpinned).

N environments: a VecEnv of N environments -- or GRL_NUM_ENVS around the script's one-factory DummyVecEnv, as for SAC -- is
stepped as one vectorised step: exploration drawn row by row in env order, the greedy rows' bins chosen on the device in one
launch (``QEngine.act_bins``, csrc/q_act.h), one ``replay_add`` of N rows, the counter advanced by N and as many updates /
target copies as multiples of ``train_freq`` / ``target_network_update_freq`` it crossed.  One environment: the loop of
stable-baselines, same random stream.

Data parallelism (BASELINE north_star: "SAC / BDQ / DQN update ... optionally sharded"):
``data_parallel="auto"`` (or GRL_DATA_PARALLEL=auto) under a torchrun launch trains one replica per rank, as ``sb.SAC``
does -- every rank steps its OWN environment and fills its own replay ring, the global minibatch is split evenly over
the ranks, the gradient SUM is exchanged inside the update's graph (``grasp_rl.parallel.DataParallelInGraph``; a
collective library as fallback), clipped per variable as the mean of the replicas and applied identically everywhere.
Counters (``num_timesteps``, exploration and beta schedules, ``learning_starts``, ``train_freq``,
``target_network_update_freq``) count environment steps of the JOB: W per loop iteration.  Callbacks, logging and
the stop decision are rank 0's.  Prioritised replay keeps one priority tree per rank (importance weights against the
rank's own total and minimum) and needs the in-graph exchange.
"""
import time

import numpy as np

from .. import _capi
from ..engine import QEngine
from . import logger
from . import policies as pol
from . import save_util
from . import spaces as sp
from .base import BaseModel, device_norm_setting, resolve_device_norm
from .callbacks import as_callback


class LinearSchedule:
    def __init__(self, schedule_timesteps, final_p, initial_p=1.0):
        self.schedule_timesteps, self.final_p, self.initial_p = max(1, int(schedule_timesteps)), final_p, initial_p

    def value(self, step):
        frac = min(float(step) / self.schedule_timesteps, 1.0)
        return self.initial_p + frac * (self.final_p - self.initial_p)


class _QModel(BaseModel):
    """Shared host loop of DQN and BDQ."""
    _engine_factory = staticmethod(lambda cfg, device: QEngine(cfg, device=device))
    algo = "dqn"

    def __init__(self, policy, env, gamma=0.99, learning_rate=5e-4, buffer_size=50000, exploration_fraction=0.1,
                 exploration_final_eps=0.02, exploration_initial_eps=1.0, train_freq=1, batch_size=32, double_q=True,
                 learning_starts=1000, target_network_update_freq=500, prioritized_replay=False,
                 prioritized_replay_alpha=0.6, prioritized_replay_beta0=0.4, prioritized_replay_beta_iters=None,
                 prioritized_replay_eps=1e-6, param_noise=False, n_cpu_tf_sess=None, verbose=0, tensorboard_log=None,
                 _init_setup_model=True, policy_kwargs=None, full_tensorboard_log=False, seed=None, device="cuda:0",
                 data_parallel=None, dp_exchange="ingraph", device_norm=None):
        if param_noise:
            raise NotImplementedError("param_noise is not implemented")
        import os
        # The VecNormalize observation statistics on the device while learning (grl_observe / grl_norm_update on the Q handle), as
        # ``sb.SAC(device_norm=...)``: every observation crosses the bus once, the loop acts on the uploaded rows (GRL_ACT_OBSERVED),
        # appends with ``replay_add_observed`` and pushes no statistics before an update.  True / False / "auto"; None reads
        # GRL_DEVICE_NORM, and for these two classes an UNSET variable means off (SAC: auto).  True and "auto" go through
        # ``resolve_device_norm``; under data parallelism the host path is taken (the Q handles do not merge their device
        # statistics over the ranks).
        self.device_norm = device_norm_setting(device_norm, unset=False)
        if data_parallel is None:
            data_parallel = os.environ.get("GRL_DATA_PARALLEL") or None
        self.data_parallel, self.dp_exchange = data_parallel, dp_exchange
        self._dp_rt = self._dp = None
        self.policy, self.policy_kwargs = policy, ({} if policy_kwargs is None else dict(policy_kwargs))
        self.gamma, self.learning_rate, self.buffer_size = gamma, learning_rate, int(buffer_size)
        self.exploration_fraction, self.exploration_final_eps = exploration_fraction, exploration_final_eps
        self.exploration_initial_eps, self.train_freq, self.batch_size = exploration_initial_eps, train_freq, int(batch_size)
        self.double_q, self.learning_starts = double_q, learning_starts
        self.target_network_update_freq = target_network_update_freq
        self.prioritized_replay, self.prioritized_replay_alpha = prioritized_replay, prioritized_replay_alpha
        self.prioritized_replay_beta0, self.prioritized_replay_beta_iters = prioritized_replay_beta0, prioritized_replay_beta_iters
        self.prioritized_replay_eps, self.param_noise = prioritized_replay_eps, param_noise
        self.verbose, self.tensorboard_log, self.seed, self.device = verbose, tensorboard_log, seed, device
        self.n_cpu_tf_sess, self.full_tensorboard_log = n_cpu_tf_sess, full_tensorboard_log
        self.num_timesteps, self.n_updates = 0, 0
        self.env = self.observation_space = self.action_space = None
        self.n_envs, self._vec_normalize_env, self.engine = 1, None, None
        self._rng = np.random.default_rng(seed)
        if self._dp_runtime() is not None:        # exploration differs per replica
            self._rng = np.random.default_rng([0 if seed is None else int(seed), self._dp_rt.rank])
        self.exploration = None
        if env is not None:
            self.set_env(env)
        if _init_setup_model and self.observation_space is not None:
            self.setup_model()

    # ------------------------------------------------------------------ model
    def _towers(self):
        raise NotImplementedError

    def setup_model(self):
        # LnMlpPolicy or policy_kwargs={"layer_norm": True}: layer normalisation in front of every hidden layer's ReLU
        # (grl_config.q_layer_norm, csrc/ln_kernels.h)
        self.layer_norm = bool(getattr(self.policy, "layer_norm", False) or self.policy_kwargs.get("layer_norm", False))
        if getattr(self.policy, "feature_extraction", "mlp") == "cnn":
            raise NotImplementedError("%s on image observations is not implemented (the reference trains it on "
                                      "auto-encoder features)" % type(self).__name__)
        # An MLP policy takes a Box of any rank: the observation is flattened in C order (tf.layers.flatten over NHWC) and NOT
        # divided by 255 -- stable-baselines 2.10's deepq FeedForwardPolicy scales only for feature_extraction == "cnn"
        # (DESIGN.md 5).  The first kernel is [prod(shape), H]; every call below hands the engine C-contiguous float32 rows.
        obs_shape = tuple(self.observation_space.shape)
        if len(obs_shape) < 1 or not sp.is_box(self.observation_space):
            raise ValueError("Box observations expected, got %s" % (self.observation_space,))
        self._obs_dim = int(np.prod(obs_shape))
        D, bins, common, branch, value = self._towers()
        vn = self._vec_normalize_env
        kw = {}
        if vn is not None:
            kw = dict(clip_obs=vn.clip_obs, clip_reward=vn.clip_reward, norm_eps=vn.epsilon)
        rt = self._dp_runtime()
        self._local_batch = self.batch_size if rt is None else rt.shard(self.batch_size, "minibatch rows")
        engine_seed = 0 if self.seed is None else int(self.seed)
        if rt is not None:
            engine_seed += 7919 * rt.rank             # every replica draws its own replay indices
            self.device = rt.device
        cfg = _capi.make_q_config(self.algo, self._obs_dim, D, bins, common, branch, value, batch_size=self._local_batch,
                                  act_batch=max(1, self.n_envs), replay_capacity=self.buffer_size, normalize=0 if vn is None else _capi.norm_mode(vn), gamma=self.gamma,
                                  lr=self._learning_rate_value(), double_q=self.double_q, seed=engine_seed,
                                  prioritized=bool(self.prioritized_replay), per_alpha=self.prioritized_replay_alpha,
                                  per_eps=self.prioritized_replay_eps, layer_norm=self.layer_norm, **kw)
        self.engine = self._engine_factory(cfg, self.device)
        self.D, self.bins = D, bins
        self._init_weights()
        if rt is not None:
            self._dp = rt.make_exchange(self.engine, prefer=self.dp_exchange)
            if self.prioritized_replay and not hasattr(self._dp, "train_per"):
                raise NotImplementedError("prioritized_replay under data parallelism needs the in-graph exchange (every rank draws "
                                          "from its own priority tree inside the update's graph); this job fell back to a collective library")
            self._dp.broadcast_parameters(src=0)
        # prioritised replay lives on the device (csrc/per_kernels.h): sampling, importance weights and the
        # priority write-back never leave HBM
        self._max_priority = 1.0

    def _init_weights(self):
        """tf.contrib.layers.fully_connected defaults: Xavier-uniform weights, zero biases; tf.contrib.layers.layer_norm
        defaults: gamma one, beta zero; target = copy."""
        rng = np.random.default_rng(0 if self.seed is None else int(self.seed))
        P = {}
        for name, _, _, shape, _ in self.engine.table:
            if "/target_q_func/" in name:
                continue
            if name.endswith("weights:0"):
                lim = np.sqrt(6.0 / (shape[0] + shape[1]))
                P[name] = rng.uniform(-lim, lim, shape).astype(np.float32)
            elif name.endswith("eps:0"):
                P[name] = np.float32(self.exploration_initial_eps).reshape(())
            elif name.endswith("/gamma:0"):
                P[name] = np.ones(shape, np.float32)
            else:
                P[name] = np.zeros(shape, np.float32)
        for name, *_ in self.engine.table:
            if "/target_q_func/" in name:
                P[name] = P[name.replace("/target_q_func", "")].copy()
        self.engine.set_parameters(P)

    def _eps_name(self):
        return ("deepq" if self.algo == "dqn" else "bdq") + "/eps:0"

    # ------------------------------------------------------------------ acting
    def _act_bins(self, obs, eps, always_draw=False):
        """Epsilon-greedy bins [n, D] of n observations.  The randomness is drawn here, row by row in env order -- one uniform
        per row (always_draw: also when eps is 0, as the learn loop does) and, only for a row that explores, its D bins: the
        stream the single-env loop consumes -- and the greedy rows are chosen on the device, one call per act_batch rows
        (engine.act_bins; skipped when every row explores)."""
        raw, observed = getattr(self, "_act_device", (False, False))    # (the learn loop, statistics on the device)
        obs = np.asarray(obs, np.float32).reshape(-1, self._obs_dim)
        explore = np.full((obs.shape[0], self.D), -1, np.int64)
        if always_draw or eps > 0:
            for i in range(obs.shape[0]):
                if self._rng.random() < eps:
                    explore[i] = self._rng.integers(0, self.bins, self.D)
        if np.all(explore >= 0):
            return explore
        if observed:      # the env wrapper uploaded these rows already (engine.observe): only the overrides and the bins move
            return self.engine.act_bins(obs.shape[0], explore, raw=raw, observed=True)
        cap = self.engine.cfg.act_batch
        kw = {"raw": True} if raw else {}
        return np.concatenate([self.engine.act_bins(obs[k:k + cap], explore[k:k + cap], **kw) for k in range(0, obs.shape[0], cap)])

    def _bins_to_env_action(self, bins):
        raise NotImplementedError

    def predict(self, observation, state=None, mask=None, deterministic=True):
        observation = np.asarray(observation)
        single = observation.shape == tuple(self.observation_space.shape)
        obs = observation.reshape((-1,) + tuple(self.observation_space.shape))
        eps = 0.0 if deterministic else float(self.engine.get_parameters()[self._eps_name()])
        acts = np.asarray([self._bins_to_env_action(b) for b in self._act_bins(obs, eps)])
        return (acts[0] if single else acts), None

    # ------------------------------------------------------------------ learn
    def learn(self, total_timesteps, callback=None, log_interval=100, tb_log_name=None, reset_num_timesteps=True,
              replay_wrapper=None):
        # (the exploration, beta and learning-rate schedules of a restored model keep the length they had in the saved run and read
        # on from the restored counter)
        total_timesteps, resume = self._begin_learn(total_timesteps, reset_num_timesteps)
        sched_total = self._schedule_total
        rt, dp = self._dp_rt, self._dp
        W = 1 if rt is None else rt.world
        lead = rt is None or rt.rank == 0
        # (decided from the callback the USER handed over; data parallel: the host path, whose moments are gathered over the ranks)
        device_norm = rt is None and self.device_norm is not False and resolve_device_norm(self.device_norm, callback, None, None)
        callback = as_callback(callback if lead else None)      # data parallel: evaluation / checkpoints / logging on rank 0 only
        callback.init_callback(self)
        eng, vn = self.engine, self._vec_normalize_env
        if rt is not None and vn is not None:       # running statistics merged over the ranks
            from ..parallel import share_running_stats
            share_running_stats(vn, rt.ctrl)
        self.exploration = LinearSchedule(self.exploration_fraction * sched_total, self.exploration_final_eps,
                                          self.exploration_initial_eps)
        beta_iters = self.prioritized_replay_beta_iters or sched_total
        beta_schedule = LinearSchedule(beta_iters, 1.0, self.prioritized_replay_beta0)
        episode_rewards, episode_successes = [0.0], []
        self.episode_reward = np.zeros((self.n_envs,))
        writer = logger.SummaryWriter(self.tensorboard_log, tb_log_name or type(self).__name__) \
            if getattr(self, "tensorboard_log", None) else None
        if device_norm and vn is not None and vn.norm_obs and eng.cfg.normalize in (1, 2):
            # restored: the device holds the statistics of the saved run already, in both halves of their double buffer
            vn.attach_device(eng, upload=resume is None)
        finished = False
        try:
            if resume is not None and vn is not None:
                obs = vn.reset_restored(resume["ret"])      # this first observation is in the restored statistics already
            else:
                obs = self.env.reset()
            obs_ = vn.get_original_obs() if vn is not None else obs
            start = time.time()
            callback.on_training_start(locals(), globals())
            callback.on_rollout_start()
            self._learn_loop(total_timesteps, callback, log_interval, rt, dp, W, lead, eng, vn, obs, obs_, beta_schedule,
                             episode_rewards, episode_successes, start)
            finished = True
        finally:
            self._act_device = (False, False)
            if vn is not None and vn._dev is not None:     # whatever ended the loop: the wrapper carries the statistics again
                vn.detach_device()
            if rt is not None and vn is not None:          # the collective hook must not outlive the collective loop
                for rms in (vn.obs_rms, vn.ret_rms):
                    rms.__dict__.pop("gather", None)
        if dp is not None and hasattr(dp, "check"):
            dp.check()                  # raises if an exchange timed out (replicas out of step)
        if dp is not None and finished and hasattr(dp, "close"):
            dp.close()                  # collective drain: no rank releases its exchange memory while a peer still pulls from it
        P = {self._eps_name(): np.float32(self.exploration.value(self.num_timesteps)).reshape(())}
        eng.set_parameters(P, exact_match=False)        # stable-baselines stores the last epsilon with the model
        callback.on_training_end()
        if writer is not None:
            writer.close()
        return self

    def _learn_loop(self, total_timesteps, callback, log_interval, rt, dp, W, lead, eng, vn, obs, obs_, beta_schedule,
                    episode_rewards, episode_successes, start):
        # stable-baselines: `for _ in range(total_timesteps)` -- a continued run (reset_num_timesteps=False) takes total_timesteps
        # MORE steps from where the counter stands; the schedules keep reading the counter itself
        end = self.num_timesteps + total_timesteps
        N = self.n_envs
        serial = vn.observed_serial if vn is not None else None     # engine.observe ticket of `obs` (device-side statistics)
        while self.num_timesteps < end:
            eps = self.exploration.value(self.num_timesteps)
            raw_obs = vn is not None and vn.hands_out_raw_observations     # (a callback may toggle vn.training)
            self._act_device = (raw_obs, raw_obs and serial is not None)
            bins = self._act_bins(obs, eps, always_draw=True)         # [N, D]: one device call for all rows
            self._act_device = (False, False)
            env_action = np.asarray([self._bins_to_env_action(b) for b in bins])
            new_obs, rew, done, info = self.env.step(env_action)
            before = self.num_timesteps
            self.num_timesteps += N * W             # environment steps of the job
            callback.update_locals(locals())
            stop = callback.on_step() is False
            if rt is not None:
                stop = rt.any(stop)                 # rank 0's callbacks decide for every replica; no rank runs ahead
            if stop:
                break
            new_serial = vn.observed_serial if vn is not None else None
            # N rows in env order.  A finished row carries done = 1, which masks the bootstrap term: the auto-reset observation
            # it holds as its next observation is never used
            if serial is not None and new_serial == serial + 1:
                # both sides of the transitions are on the device already (uploaded once each by the wrapper)
                new_obs_, rew_ = vn.old_obs, vn.old_rews
                eng.replay_add_observed(bins.astype(np.float32).reshape(N, -1), rew_, done)
            else:
                new_obs_, rew_ = (vn.get_original_obs(), vn.get_original_reward()) if vn is not None else (new_obs, rew)
                eng.replay_add(np.asarray(obs_, np.float32), bins.astype(np.float32).reshape(N, -1),
                               np.asarray(rew_, np.float32), np.asarray(new_obs_, np.float32), np.asarray(done, np.float32))
            obs, obs_, serial = new_obs, new_obs_, new_serial
            self.episode_reward += np.asarray(rew_, np.float64).reshape(N)
            for i in range(N):
                if done[i] and isinstance(info[i], dict) and info[i].get("is_success") is not None:
                    episode_successes.append(float(info[i]["is_success"]))
            episode_rewards[-1] += float(np.asarray(rew_).reshape(-1)[0])
            if done[0]:
                episode_rewards.append(0.0)
            can_sample = eng.replay_size() >= self._local_batch
            # one update per train_freq environment steps of the job: W of them happened in this iteration
            crossed = lambda every: self.num_timesteps // max(1, int(every)) - before // max(1, int(every))
            n_upd = crossed(self.train_freq) if (can_sample and self.num_timesteps > self.learning_starts) else 0
            if n_upd > 0:
                callback.on_rollout_end()
                if vn is not None and eng.cfg.normalize:
                    if vn.hands_out_raw_observations:     # observation statistics live on the device: only the return variance moves
                        eng.set_ret_var(float(vn.ret_rms.var))
                    else:
                        eng.set_obs_stats(vn.obs_rms.mean, vn.obs_rms.var, float(vn.ret_rms.var))
                if callable(self.learning_rate):    # stable-baselines evaluates the schedule per update: lr(1 - step / total)
                    eng.set_learning_rate(self.learning_rate(1.0 - (self.num_timesteps - 1) / max(1, self._schedule_total)))
                if self.prioritized_replay:
                    (eng if dp is None else dp).train_per(n_upd, beta_schedule.value(self.num_timesteps))
                elif dp is not None:
                    dp.train(n_upd)                # the global minibatch: gradients exchanged inside each update's graph
                else:
                    eng.train(n_upd)               # uniform indices from the device RNG, importance weights 1
                self.n_updates += n_upd
                callback.on_rollout_start()
            if can_sample and self.num_timesteps > self.learning_starts and crossed(self.target_network_update_freq) > 0:
                eng.update_target()
            if self.verbose >= 1 and lead and done[0] and log_interval is not None and len(episode_rewards) % log_interval == 0:
                logger.logkv("steps", self.num_timesteps)
                logger.logkv("episodes", len(episode_rewards))
                logger.logkv("mean 100 episode reward", round(float(np.mean(episode_rewards[-101:-1])), 1))
                logger.logkv("% time spent exploring", int(100 * eps))
                if episode_successes:
                    logger.logkv("success rate", float(np.mean(episode_successes[-100:])))
                logger.logkv("fps", int(self.num_timesteps / (time.time() - start + 1e-9)))
                logger.dumpkvs()

    # ------------------------------------------------------------------ persistence
    _SAVED = ("double_q", "param_noise", "learning_starts", "train_freq", "prioritized_replay",
              "prioritized_replay_eps", "batch_size", "target_network_update_freq", "prioritized_replay_alpha",
              "prioritized_replay_beta0", "prioritized_replay_beta_iters", "exploration_final_eps",
              "exploration_fraction", "gamma", "verbose", "buffer_size", "n_cpu_tf_sess", "seed", "policy_kwargs")

    def _data(self):
        d = {k: getattr(self, k) for k in self._SAVED}
        if getattr(self, "layer_norm", False):      # the zip rebuilds the same network whichever way it was asked for
            d["policy_kwargs"] = dict(self.policy_kwargs, layer_norm=True)
        d["learning_rate"] = self._learning_rate_value()
        d.update(observation_space=self.observation_space, action_space=self.action_space, policy=self.policy,
                 n_envs=self.n_envs, _vectorize_action=True)
        return d

    def _save_zip(self, save_path):
        return save_util.save_to_zip(save_path, self._data(), self.get_parameters())

    @classmethod
    def _load_zip(cls, load_path, env=None, custom_objects=None, **kwargs):
        data, params = save_util.load_from_zip(load_path)
        model = cls(policy=data.get("policy") if isinstance(data.get("policy"), type) else None, env=None,
                    _init_setup_model=False)
        for k, v in data.items():
            if k in cls._SAVED + ("learning_rate", "num_actions_pad", "epsilon_greedy") and v is not None:
                setattr(model, k, v)
        return model._finish_load(data, params, env, kwargs)

    def _host_state(self, include_replay):
        return dict(super()._host_state(include_replay), max_priority=self._max_priority,
                    exploration_eps=None if self.exploration is None else float(self.exploration.value(self.num_timesteps)))

    def _restore_host_state(self, st):
        super()._restore_host_state(st)
        self._max_priority = st["max_priority"]


class DQN(_QModel):
    """Stock stable-baselines deepq: two separate dueling towers on the observation."""
    algo = "dqn"

    def _towers(self):
        if not sp.is_discrete(self.action_space):
            raise ValueError("DQN needs a Discrete action space")
        if not self.policy_kwargs.get("dueling", True):
            raise NotImplementedError("only the dueling architecture (stable-baselines default) is implemented")
        layers = tuple(self.policy_kwargs.get("layers", (64, 64)))
        return 1, int(self.action_space.n), (), layers, layers

    def _bins_to_env_action(self, bins):
        return int(bins[0])


class BDQ(_QModel):
    """Branching dueling Q-network of the reference's ``bdq_sb`` fork (decisions: SURVEY.md A.6)."""
    algo = "bdq"

    def __init__(self, policy, env, num_actions_pad=33, epsilon_greedy=True, learning_rate=1e-4, batch_size=64,
                 buffer_size=1000000, target_network_update_freq=1000, exploration_fraction=0.1,
                 exploration_final_eps=0.02, **kwargs):
        self.num_actions_pad, self.epsilon_greedy = int(num_actions_pad), epsilon_greedy
        if not epsilon_greedy:
            raise NotImplementedError("only epsilon-greedy exploration is implemented for BDQ")
        super().__init__(policy, env, learning_rate=learning_rate, batch_size=batch_size, buffer_size=buffer_size,
                         target_network_update_freq=target_network_update_freq,
                         exploration_fraction=exploration_fraction, exploration_final_eps=exploration_final_eps, **kwargs)

    _SAVED = _QModel._SAVED + ("num_actions_pad", "epsilon_greedy")

    def _towers(self):
        if not sp.is_box(self.action_space):
            raise ValueError("BDQ discretises a continuous (Box) action space")
        layers = self.policy_kwargs.get("layers", [[512, 256], [128], [128]])
        if len(layers) != 3:
            raise ValueError("policy_kwargs['layers'] must be [[common...], [branch...], [value...]]")
        return int(np.prod(self.action_space.shape)), self.num_actions_pad, tuple(layers[0]), tuple(layers[1]), tuple(layers[2])

    def _bins_to_env_action(self, bins):
        low, high = np.asarray(self.action_space.low, np.float32), np.asarray(self.action_space.high, np.float32)
        unit = -1.0 + 2.0 * np.asarray(bins, np.float32) / float(self.bins - 1)       # bin k -> [-1, 1]
        return (low + 0.5 * (unit + 1.0) * (high - low)).reshape(self.action_space.shape)
