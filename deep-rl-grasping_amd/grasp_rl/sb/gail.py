"""``GAIL`` of stable-baselines 2.10.1 (``gail/model.py``): TRPO with a reward giver.  The generator is ``TRPO`` unchanged (trpo.py,
csrc/plan_trpo.inl); the discriminator -- ``TransitionClassifier`` on Box actions, its running input statistics, its Adam -- is a
session on the TRPO handle (``TrpoEngine.gail_*``; csrc/plan_gail.inl, csrc/gail_kernels.h), and everything that touches a tensor
runs there.  This file is the host half of the ``using_gail`` branches of ``trpo_mpi.py``:

  * a rollout of ``timesteps_per_batch`` steps is collected as TRPO collects it; before GAE is formed its rewards are replaced by
    ``-log(1 - sigmoid(D(obs, clip(action))) + 1e-8)`` in ONE batched pass on the device (the discriminator does not change during
    a rollout, so this is the per-step evaluation of stable-baselines).  The environment's reward is kept for the log only:
    ``EpRewMean`` is over discriminator returns, ``EpTrueRewMean`` over true returns;
  * every ``g_step``-th iteration the discriminator is updated on the LAST rollout: its T rows are shuffled with the model's
    seeded generator and cut into ``T // (T // d_step)`` minibatches of ``T // d_step`` rows (the tail is dropped; observations
    and UNCLIPPED policy actions), each paired with ``expert_dataset.get_next_batch()`` -- handed to the device as row indices of
    the table uploaded once per ``learn``; the six losses are logged as their means over the minibatches.

``num_timesteps`` grows by ``timesteps_per_batch`` per rollout, as TRPO's does.  Deviation from stable-baselines, also stated in
INTEGRATION.md: the expert dataset is NEVER pickled into the zip -- the zip is TRPO's with ``using_gail=True`` and
``expert_dataset=None``; ``GAIL.load(path, env, expert_dataset=ds)`` sets it.  The adversary is not saved, as in stable-baselines:
a loaded model starts a fresh one.  Refused by name: everything TRPO refuses (Discrete actions, more than one environment, ...),
``learn`` without a dataset, a dataset whose observation / action widths do not fit the spaces, ``save_checkpoint`` /
``load_checkpoint`` (a session is not in a checkpoint; with GRL_CHECKPOINT_STATE=1 ``save`` writes the zip only and says why)."""
import numpy as np

from . import logger
from .trpo import TRPO


def glorot_adversary(shapes, seed):
    """Glorot-uniform weights, zero biases (tf.contrib.layers.fully_connected) from a generator seeded like the model."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shape in shapes.items():
        if len(shape) == 2:
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            out[name] = rng.uniform(-lim, lim, shape).astype(np.float32)
        else:
            out[name] = np.zeros(shape, np.float32)
    return out


class GAIL(TRPO):
    def __init__(self, policy, env, expert_dataset=None, hidden_size_adversary=100, adversary_entcoeff=1e-3, g_step=3, d_step=1,
                 d_stepsize=3e-4, verbose=0, _init_setup_model=True, **kwargs):
        refused = sorted(set(kwargs) & {"using_gail", "reward_giver"})
        if refused:
            raise TypeError("GAIL: unexpected keyword arguments %s (GAIL sets them itself)" % refused)
        super().__init__(policy, env, verbose=verbose, _init_setup_model=False, **kwargs)
        self.using_gail = True
        self.expert_dataset = expert_dataset
        self.g_step, self.d_step, self.d_stepsize = int(g_step), int(d_step), float(d_stepsize)
        self.hidden_size_adversary, self.adversary_entcoeff = int(hidden_size_adversary), float(adversary_entcoeff)
        self.true_rew_buffer = type(self.rew_buffer)(maxlen=40)
        self._cur_disc_ret, self._ep_true_rets, self._table = 0.0, [], None
        self.last_d_losses = None
        if _init_setup_model and self.observation_space is not None:
            self.setup_model()

    # ------------------------------------------------------------------ model
    def setup_model(self):
        if not 1 <= self.hidden_size_adversary <= 1024:
            raise NotImplementedError("GAIL: hidden_size_adversary must be 1..1024, got %d" % self.hidden_size_adversary)
        if self.g_step < 1 or not 1 <= self.d_step <= self.timesteps_per_batch:
            raise NotImplementedError("GAIL: g_step must be >= 1 and d_step 1..timesteps_per_batch, got %d and %d" % (self.g_step, self.d_step))
        super().setup_model()
        eng = self.engine
        self.d_batch = self.timesteps_per_batch // self.d_step
        eng.gail_begin(self.hidden_size_adversary, self.d_batch, self.adversary_entcoeff, self.d_stepsize,
                       np.broadcast_to(self.action_space.low, self.action_space.shape), np.broadcast_to(self.action_space.high, self.action_space.shape))
        eng.gail_set_parameters(glorot_adversary(eng.gail_param_shapes(), 0 if self.seed is None else int(self.seed)))

    def _check_dataset(self):
        ds = self.expert_dataset
        if ds is None:
            raise ValueError("GAIL: learn needs an expert dataset (GAIL(..., expert_dataset=ds) or GAIL.load(path, env, expert_dataset=ds))")
        if ds.observations.shape[1] != self._obs_dim or ds.actions.shape[1] != self._act_dim:
            raise ValueError("GAIL: the expert dataset holds observations of %d and actions of %d values, the spaces %d and %d"
                             % (ds.observations.shape[1], ds.actions.shape[1], self._obs_dim, self._act_dim))
        return ds

    # ------------------------------------------------------------------ learn
    def learn(self, total_timesteps, callback=None, log_interval=100, tb_log_name="GAIL", reset_num_timesteps=True):
        ds = self._check_dataset()
        ds.init_dataloader(self.d_batch)
        self._table = self.engine.gail_upload(ds.observations, ds.actions)
        self._cur_disc_ret = 0.0
        try:
            return self._learn(total_timesteps, callback, log_interval, tb_log_name, reset_num_timesteps)
        finally:
            self.engine.synchronize()
            self._table = None

    def _before_finish(self, eng, episode_start, ep_rets):
        """Rewards on the device, then the T rewards back so that ``ep_rets`` holds discriminator returns; the true returns the
        loop accumulated go to a buffer of their own."""
        T = self.timesteps_per_batch
        eng.gail_rewards()
        rew, es = eng.fetch("ppo_rew", (T,)), eng.fetch("ppo_done", (T,))
        ends = np.append(es[1:], episode_start[0]) > 0      # an episode ends behind step t where the next step starts one
        self._ep_true_rets = list(ep_rets)
        del ep_rets[:]
        cur = self._cur_disc_ret
        for t in range(T):
            cur += float(rew[t])
            if ends[t]:
                ep_rets.append(cur)
                cur = 0.0
        self._cur_disc_ret = cur

    def _after_update(self, eng, iters_so_far):
        T, b = self.timesteps_per_batch, self.d_batch
        self.true_rew_buffer.extend(self._ep_true_rets)
        if (iters_so_far + 1) % self.g_step == 0:
            n_mb = T // b
            gen = self._rng.permutation(T)[:n_mb * b].reshape(n_mb, b).astype(np.int32)
            exp = np.full((n_mb, b), -1, np.int32)
            for k in range(n_mb):
                ix = self.expert_dataset.dataloader.next_indices()
                exp[k, :len(ix)] = ix
            eng.gail_update(self._table, gen, exp)
            if self.verbose >= 1:
                self.last_d_losses = eng.gail_losses().mean(axis=0)
                for name, val in zip(eng.LOSS_NAMES, self.last_d_losses):
                    logger.logkv(name, float(val))
        if self.verbose >= 1 and len(self.true_rew_buffer) > 0:
            logger.logkv("EpTrueRewMean", float(np.mean(self.true_rew_buffer)))

    # ------------------------------------------------------------------ persistence
    def _save_zip(self, save_path):
        ds, self.expert_dataset = self.expert_dataset, None      # never pickled into the zip
        try:
            return super()._save_zip(save_path)
        finally:
            self.expert_dataset = ds

    def save(self, save_path, cloudpickle=False):
        from . import checkpoint
        if checkpoint.enabled():
            logger.warn("GAIL: GRL_CHECKPOINT_STATE=1 is set, but a GAIL session (discriminator, its statistics and optimiser) is not "
                        "in a checkpoint: writing the zip only")
        return self._save_zip(save_path)

    @classmethod
    def load(cls, load_path, env=None, custom_objects=None, **kwargs):
        model = cls._load_zip(load_path, env=env, custom_objects=custom_objects, **kwargs)
        model.using_gail = True
        return model

    def save_checkpoint(self, path, include_replay=True):
        raise NotImplementedError("GAIL: save_checkpoint is not implemented (a GAIL session is not in a checkpoint)")

    @classmethod
    def load_checkpoint(cls, path, env=None, **kwargs):
        raise NotImplementedError("GAIL: load_checkpoint is not implemented (a GAIL session is not in a checkpoint)")
