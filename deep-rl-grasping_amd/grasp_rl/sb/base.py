"""``BaseModel``: what ``SAC``, ``DQN``, ``BDQ``, ``PPO2`` and ``TRPO`` share of the stable-baselines model surface, each piece
once -- the environment plumbing (``set_env`` and its two hooks), the data-parallel runtime, the ``device_norm`` setting, the
parameter accessors, the first statements of every ``learn`` and the last ones of every ``_load_zip``.  ``save`` / ``load`` and the
full-state checkpoints come from ``CheckpointMixin`` (sb/checkpoint.py); what only the two on-policy models share is
``OnPolicyModel`` (sb/on_policy.py).  A model class provides ``_engine_factory``, its constructor, ``setup_model``, ``learn``,
``predict``, ``_save_zip`` and ``_load_zip``.
"""
import os

from . import logger
from . import save_util
from .callbacks import as_callback, may_read_observations
from .checkpoint import CheckpointMixin
from .vec_env import DummyVecEnv, VecEnv, expand_training_env, unwrap_vec_normalize


def resolve_device_norm(setting, user_callback, rt, dp):
    """Where the VecNormalize statistics live during ``learn``: True = on the device (``grl_observe`` / ``grl_norm_update``).
    'auto' looks at the callback the USER handed over -- before ``learn`` replaces it by a bare one on ranks > 0 -- and under
    data parallelism the decision is COLLECTIVE (``rt.all``): with the statistics on the device every env step runs an
    in-kernel merge that waits for all peers, with them on the host an all_gather on the control group; replicas that chose
    differently (a script that hands only rank 0 a callback) would wait for each other in two different exchanges."""
    if setting == "auto":
        setting = not (user_callback is not None and may_read_observations(as_callback(user_callback)))
    setting = bool(setting)
    if rt is not None:
        if setting and not hasattr(dp, "check"):
            # the device-side merge of the statistics rides on the in-graph exchange's channel; with the collective
            # fallback (RCCL / gloo) the handle is not connected and every replica would keep its own observation
            # statistics: take the host path, whose moments are gathered over the ranks
            logger.warn("device_norm needs the in-graph exchange; this job fell back to a collective library -> host statistics")
            setting = False
        setting = rt.all(setting)
    return setting


def device_norm_setting(device_norm, unset):
    """The ``device_norm`` keyword of every model: True, False or 'auto'.  None reads GRL_DEVICE_NORM (0 / 1 / auto); `unset` is
    what the class takes when the variable is not set (or holds anything else): 'auto' for SAC, False for the other models."""
    if device_norm is None:
        device_norm = {"0": False, "1": True, "auto": "auto"}.get(os.environ.get("GRL_DEVICE_NORM"), unset)
    return device_norm if device_norm == "auto" else bool(device_norm)


class BaseModel(CheckpointMixin):
    data_parallel = None      # PPO2 / TRPO: always one replica
    _dp_rt = _dp = None

    # ------------------------------------------------------------------ environment
    def set_env(self, env):
        if env is not None and not isinstance(env, VecEnv) and not hasattr(env, "num_envs"):
            env = DummyVecEnv([lambda: env])
        if env is not None:
            env = self._training_env(env)
            if self.observation_space is not None and tuple(env.observation_space.shape) != tuple(self.observation_space.shape):
                raise ValueError("observation space of the new env does not match the model")
            if self.engine is not None:
                self._check_fits_engine(env)
            self.observation_space, self.action_space = env.observation_space, env.action_space
            self.n_envs = env.num_envs
            self._vec_normalize_env = unwrap_vec_normalize(env)
        self.env = env

    def _training_env(self, env):
        """The env this model trains on.  GRL_NUM_ENVS: the env a model is handed is its TRAINING env -- the one the reference's
        script wraps as DummyVecEnv([one factory]) (train_stable_baselines.py:52-54) fans out to worker processes here (row J3);
        under data parallelism to this process's share of the job's environments."""
        rt = self._dp_runtime()
        return expand_training_env(env, rank=0 if rt is None else rt.rank, world=1 if rt is None else rt.world)

    def _check_fits_engine(self, env):
        if env.num_envs > self.engine.cfg.act_batch:
            raise ValueError("env has more sub-environments than the model was built for")

    def get_env(self):
        return self.env

    def get_vec_normalize_env(self):
        return self._vec_normalize_env

    # ------------------------------------------------------------------ data parallel
    def _dp_runtime(self):
        if self._dp_rt is not None:
            return self._dp_rt
        if self.data_parallel in (None, False, "", "0", "off"):
            return None
        from ..parallel import runtime_for
        self._dp_rt = runtime_for(self.data_parallel)
        return self._dp_rt

    # ------------------------------------------------------------------ learn
    def _learning_rate_value(self):
        lr = self.learning_rate
        return float(lr(1.0)) if callable(lr) else float(lr)

    def pretrain(self, dataset, n_epochs=10, learning_rate=1e-4, adam_epsilon=1e-8, val_interval=None):
        raise NotImplementedError("%s: pretrain is not implemented (behaviour cloning runs on SAC models only)" % type(self).__name__)

    def _begin_learn(self, total_timesteps, reset_num_timesteps):
        """The first statements of every ``learn``: (total_timesteps as an int, the restored position or None).  A model restored
        from a checkpoint continues in place (sb/checkpoint.py): its counters, the schedules' reference length and the
        statistics stand where the saved run left them."""
        if self.env is None:
            raise ValueError("learn() needs an environment")
        total_timesteps = int(total_timesteps)      # (the reference's --timestep arrives as a string)
        if reset_num_timesteps:
            self.num_timesteps = 0
        resume = self._take_resume(reset_num_timesteps)
        self._schedule_total = total_timesteps if resume is None else (resume["schedule_total"] or total_timesteps)
        return total_timesteps, resume

    # ------------------------------------------------------------------ parameters / persistence
    def get_parameter_list(self):
        return self.engine.param_names()

    def get_parameters(self):
        return self.engine.get_parameters()

    def load_parameters(self, load_path_or_dict, exact_match=True):
        params = load_path_or_dict
        if isinstance(params, str):
            _, params = save_util.load_from_zip(params)
        elif isinstance(params, (list, tuple)):
            params = dict(zip(self.get_parameter_list(), params))
        known = set(self.get_parameter_list())
        unknown = [k for k in params if k not in known]
        if unknown:
            raise RuntimeError("load_parameters: unknown parameter(s) %s" % unknown[:5])
        self.engine.set_parameters(params, exact_match=exact_match)

    def _finish_load(self, data, params, env, kwargs):
        """The last statements of every ``_load_zip``, on the model it made and filled from ``data``: the caller's keyword
        overrides, the spaces (the zip's, or those of `env`), the engine and the parameters."""
        self.policy_kwargs = dict(self.policy_kwargs or {})
        for k, v in kwargs.items():
            setattr(self, k, v)
        self.observation_space, self.action_space = data.get("observation_space"), data.get("action_space")
        if env is not None:
            self.set_env(env)
        if self.observation_space is None or self.action_space is None:
            raise ValueError("the zip holds no readable spaces; pass env=")
        self._before_setup(data, params)
        self.setup_model()
        self.load_parameters(params)
        return self

    def _before_setup(self, data, params):
        """What a loaded model takes from the zip once the caller's overrides are in and before the engine is built."""
