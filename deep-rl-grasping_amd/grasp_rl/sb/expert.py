"""``ExpertDataset`` and ``generate_expert_traj`` of stable-baselines 2.10 (``stable_baselines.gail``): recorded
(observation, action) pairs for ``model.pretrain``.  Arrays only: the dataset lives in host memory as two float32 tables and a
loader is an index order over its split, so nothing here needs worker processes (``sequential_preprocessing`` is accepted and
changes nothing).  Image observations are recorded as arrays, never as files: a dataset of image paths and a non-default
``image_folder`` are refused by name.

The ``.npz`` format is stable-baselines': ``actions``, ``obs``, ``rewards``, ``episode_returns``, ``episode_starts``."""
import numpy as np

from .vec_env import VecEnv

KEYS = ("actions", "obs", "rewards", "episode_returns", "episode_starts")
DEFAULT_IMAGE_FOLDER = "recorded_images"


class DataLoader:
    """An order over ``indices`` of the dataset's tables, cut into minibatches of ``batch_size`` (the last one may be shorter).
    Iterating yields (observations, actions) like stable-baselines' loader; ``index_rows()`` is the same epoch as the
    engine takes it: int32 [len(self), batch_size], a shorter last minibatch ending in -1; ``next_indices()`` is ``next()``
    as indices."""

    def __init__(self, indices, observations, actions, batch_size, shuffle=True):
        self.indices = np.asarray(indices, np.int64).copy()
        self.observations, self.actions = observations, actions
        self.batch_size, self.shuffle = int(batch_size), bool(shuffle)
        self.n_minibatches = (len(self.indices) + self.batch_size - 1) // self.batch_size
        self._it = None

    def __len__(self):
        return self.n_minibatches

    def _epoch_order(self):
        return np.random.permutation(self.indices) if self.shuffle else self.indices

    def index_rows(self):
        order = self._epoch_order()
        rows = np.full((self.n_minibatches, self.batch_size), -1, np.int32)
        rows.reshape(-1)[:len(order)] = order
        return rows

    def _epoch_indices(self):
        order = self._epoch_order()
        for k in range(0, len(order), self.batch_size):
            yield order[k:k + self.batch_size]

    def __iter__(self):
        for ix in self._epoch_indices():
            yield self.observations[ix], self.actions[ix]

    def next_indices(self):
        """The table rows of the batch ``__next__`` would hand out (the same ``np.random`` draws, the same cursor): GAIL gathers
        them on the device."""
        if self._it is None:
            self._it = self._epoch_indices()
        try:
            return next(self._it)
        except StopIteration:
            self._it = self._epoch_indices()
            return next(self._it)

    def __next__(self):
        ix = self.next_indices()
        return self.observations[ix], self.actions[ix]


class ExpertDataset:
    def __init__(self, expert_path=None, traj_data=None, train_fraction=0.7, batch_size=64, traj_limitation=-1, randomize=True,
                 verbose=1, sequential_preprocessing=False):
        if traj_data is not None and expert_path is not None:
            raise ValueError("Cannot specify both 'traj_data' and 'expert_path'")
        if traj_data is None and expert_path is None:
            raise ValueError("Must specify one of 'traj_data' or 'expert_path'")
        if traj_data is None:
            with np.load(expert_path, allow_pickle=True) as z:
                traj_data = {k: z[k] for k in z.files}
        missing = [k for k in KEYS if k not in traj_data]
        if missing:
            raise ValueError("ExpertDataset: the trajectory data lacks %s" % missing)
        obs, actions = np.asarray(traj_data["obs"]), np.asarray(traj_data["actions"])
        if obs.dtype.kind in "USO":
            raise NotImplementedError("ExpertDataset: image paths (string observations) are not implemented; record the "
                                      "observations as arrays (generate_expert_traj does)")
        episode_starts = np.asarray(traj_data["episode_starts"]).astype(bool).reshape(-1)
        limit = len(obs)
        if traj_limitation > 0:
            n_episodes = 0
            for i, start in enumerate(episode_starts):
                n_episodes += int(start)
                if n_episodes == traj_limitation + 1:
                    limit = i
                    break
        self.observations = np.ascontiguousarray(obs[:limit], np.float32).reshape(limit, -1)
        self.actions = np.ascontiguousarray(actions[:limit], np.float32).reshape(limit, -1)
        self.obs_shape = tuple(obs.shape[1:])
        order = np.random.permutation(limit).astype(np.int64)
        n_train = int(train_fraction * limit)
        self.train_indices, self.val_indices = order[:n_train], order[n_train:]
        if len(self.train_indices) == 0:
            raise ValueError("No sample for the training set")
        if len(self.val_indices) == 0:
            raise ValueError("No sample for the validation set")
        self.returns = np.asarray(traj_data["episode_returns"])[:traj_limitation if traj_limitation > 0 else None]
        self.avg_ret = float(np.mean(self.returns)) if len(self.returns) else 0.0
        self.std_ret = float(np.std(self.returns)) if len(self.returns) else 0.0
        self.num_traj = int(min(traj_limitation, episode_starts.sum()) if traj_limitation > 0 else episode_starts.sum())
        self.num_transition = limit
        self.verbose, self.randomize, self.batch_size = verbose, bool(randomize), int(batch_size)
        self.sequential_preprocessing = sequential_preprocessing
        self.dataloader = None
        self.train_loader = DataLoader(self.train_indices, self.observations, self.actions, batch_size, shuffle=self.randomize)
        self.val_loader = DataLoader(self.val_indices, self.observations, self.actions, batch_size, shuffle=self.randomize)
        if self.verbose >= 1:
            self.log_info()

    def init_dataloader(self, batch_size):
        """The loader over the WHOLE dataset that get_next_batch(None) draws from (GAIL's use)."""
        self.dataloader = DataLoader(np.concatenate([self.train_indices, self.val_indices]), self.observations, self.actions,
                                     batch_size, shuffle=self.randomize)

    def get_next_batch(self, split=None):
        loader = {None: self.dataloader, "train": self.train_loader, "val": self.val_loader}[split]
        if loader is None:
            raise ValueError("init_dataloader(batch_size) first")
        return next(loader)

    def log_info(self):
        print("Total trajectories: {}".format(self.num_traj))
        print("Total transitions: {}".format(self.num_transition))
        print("Average returns: {}".format(self.avg_ret))
        print("Std for returns: {}".format(self.std_ret))

    def prepare_pickling(self):
        self.dataloader, self.train_loader._it, self.val_loader._it = None, None, None


def generate_expert_traj(model, save_path=None, env=None, n_timesteps=0, n_episodes=100, image_folder=DEFAULT_IMAGE_FOLDER):
    """Runs `model` (a model of this package, or a callable obs -> action) for n_episodes in `env` (default: the model's own)
    and records what the environment hands out -- through a VecNormalize wrapper that is the normalised observation.
    n_timesteps > 0 trains the model first.  Returns the dict of the five arrays and writes it to save_path(.npz)."""
    if image_folder != DEFAULT_IMAGE_FOLDER:
        raise NotImplementedError("generate_expert_traj: image_folder is not implemented (observations are recorded as arrays, "
                                  "never as image files)")
    if env is None and hasattr(model, "get_env"):
        env = model.get_env()
    if env is None:
        raise ValueError("You must set the env in the model or pass it to the function.")
    is_vec = isinstance(env, VecEnv) or hasattr(env, "num_envs")
    if is_vec and env.num_envs != 1:
        raise ValueError("generate_expert_traj: you must use a single environment")
    if n_timesteps > 0 and hasattr(model, "learn"):
        model.learn(n_timesteps)
    act = (lambda o: model.predict(o)[0]) if hasattr(model, "predict") else model
    observations, actions, rewards, episode_starts = [], [], [], [True]
    episode_returns = np.zeros(n_episodes)
    obs, ret, ep = env.reset(), 0.0, 0
    while ep < n_episodes:
        observations.append(np.array(obs[0] if is_vec else obs, copy=True))
        action = act(obs)
        obs, reward, done, _ = env.step(action)
        if is_vec:
            action, reward, done = np.asarray(action)[0], np.asarray(reward)[0], bool(np.asarray(done)[0])
        actions.append(np.array(action, copy=True))
        rewards.append(float(reward))
        episode_starts.append(bool(done))
        ret += float(reward)
        if done:
            if not is_vec:
                obs = env.reset()
            episode_returns[ep], ret, ep = ret, 0.0, ep + 1
    out = {"actions": np.stack(actions).reshape((len(actions),) + tuple(env.action_space.shape)),
           "obs": np.stack(observations).reshape((len(observations),) + tuple(env.observation_space.shape)),
           "rewards": np.asarray(rewards), "episode_returns": episode_returns,
           "episode_starts": np.asarray(episode_starts[:-1])}
    if save_path is not None:
        np.savez(save_path, **out)
    return out
