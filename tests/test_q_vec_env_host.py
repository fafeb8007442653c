"""DQN / BDQ on N environments (grasp_rl/sb/dqn.py) on the g++ emulation build of the engine: counters, the order in which
transitions reach the replay ring and updates follow them, the unchanged single-environment run, what the ring holds, and
predict on more rows than act_batch.  The emulated `grl_act(GRL_ACT_GREEDY)` runs tests/hostemu/q_act_ref1.h."""
import functools

import numpy as np
import pytest

import stable_baselines as sb
from fake_env import FakeGraspEnv
from grasp_rl.engine import QEngine
from grasp_rl.sb.callbacks import BaseCallback
from grasp_rl.sb.dqn import BDQ, DQN, LinearSchedule
from hostemu_backend import NumpyHostBackend
from stable_baselines.bdq.policies import MlpActPolicy
from stable_baselines.common.vec_env import DummyVecEnv
from stable_baselines.deepq.policies import MlpPolicy as DQNMlpPolicy

OBS_DIM, N_ENVS, TOTAL = 20, 4, 96          # 24 vectorised steps of 4 environments
EPISODE_LEN = (3, 5, 7, 4)                  # episodes end in different rows at different steps


@pytest.fixture
def emulated_q_engine(hostemu_lib, monkeypatch):
    f = staticmethod(lambda cfg, device: QEngine(cfg, backend=NumpyHostBackend(), lib_path=hostemu_lib))
    monkeypatch.setattr(DQN, "_engine_factory", f)
    monkeypatch.setattr(BDQ, "_engine_factory", f)


class Recorder(FakeGraspEnv):
    """FakeGraspEnv that keeps what it handed out: observations (reset and step), and per step (action, reward, done)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen_obs, self.seen_steps = [], []

    def reset(self):
        o = super().reset()
        self.seen_obs.append(o.copy())
        return o

    def step(self, action):
        o, r, d, info = super().step(action)
        self.seen_obs.append(o.copy())
        self.seen_steps.append((np.array(action, np.float32, copy=True), r, d))
        return o, r, d, info


class StepCounter(BaseCallback):
    def __init__(self):
        super().__init__()
        self.steps = 0

    def _on_step(self):
        self.steps += 1
        return True


def make_env(algo, k, cls=FakeGraspEnv):
    kw = dict(discrete_actions=6) if algo == "dqn" else dict(act_dim=3)
    return cls(seed=10 + k, vector_dim=OBS_DIM, episode_len=EPISODE_LEN[k % 4], **kw)


def make_model(algo, env, per=False, **kw):
    common = dict(gamma=0.99, batch_size=8, buffer_size=kw.pop("buffer_size", 64), learning_starts=10,
                  target_network_update_freq=10, prioritized_replay=per, seed=3, **kw)
    if algo == "dqn":
        return sb.DQN(DQNMlpPolicy, env, policy_kwargs={"layers": [16, 16]}, **common)
    return sb.BDQ(MlpActPolicy, env, policy_kwargs={"layers": [[16, 16], [8], [8]]}, num_actions_pad=5,
                  exploration_fraction=0.3, exploration_final_eps=0.1, **common)


def expected_schedule(model, n_envs, total, capacity):
    """The rule of the learn loop, restated: per vectorised step the counter advances by n_envs, the ring by n_envs rows;
    updates / target copies = multiples of train_freq / target_network_update_freq the counter crossed, once a minibatch can
    be drawn and the counter is beyond learning_starts.  Returns [(n_updates, copy_target, counter)] per step."""
    out, ts, size = [], 0, 0
    while ts < total:
        before, ts, size = ts, ts + n_envs, min(capacity, size + n_envs)
        ok = size >= model.batch_size and ts > model.learning_starts
        crossed = lambda every: ts // every - before // every
        out.append((crossed(model.train_freq) if ok else 0, ok and crossed(model.target_network_update_freq) > 0, ts))
    return out


@pytest.mark.parametrize("fan_out", [False, True])
@pytest.mark.parametrize("algo", ["dqn", "bdq"])
def test_learns_on_four_environments(emulated_q_engine, monkeypatch, algo, fan_out):
    """Four environments -- a 4-factory DummyVecEnv, or GRL_NUM_ENVS=4 around the one-factory DummyVecEnv of the reference's
    script -- advance the counter by 4 per vectorised step; updates, ring and callback steps follow the rule."""
    if fan_out:
        monkeypatch.setenv("GRL_NUM_ENVS", "4")
        monkeypatch.setenv("GRL_ENV_START_METHOD", "fork")      # (the emulation engine has no HIP context a fork could damage)
        env = DummyVecEnv([functools.partial(make_env, algo, 0)])
    else:
        env = DummyVecEnv([functools.partial(make_env, algo, k) for k in range(N_ENVS)])
    try:
        model = make_model(algo, env)
        assert model.n_envs == N_ENVS and model.engine.cfg.act_batch == N_ENVS and model.get_env().num_envs == N_ENVS
        counter = StepCounter()
        p0 = model.get_parameters()
        model.learn(total_timesteps=TOTAL, callback=counter)
        sched = expected_schedule(model, N_ENVS, TOTAL, 64)
        assert model.num_timesteps == TOTAL and counter.steps == TOTAL // N_ENVS == len(sched)
        assert model.n_updates == sum(s[0] for s in sched) == 88
        assert model.engine.replay_size() == 64
        p1 = model.get_parameters()
        assert sum(not np.array_equal(p0[k], p1[k]) for k in p0 if "target_q_func" not in k and "eps" not in k) > 4
        tgt = [k for k in p1 if "target_q_func" in k and k.endswith("weights:0")][0]
        assert not np.array_equal(p0[tgt], p1[tgt])
    finally:
        env.close()


def _spy_replay(model):
    rows, real = [], model.engine.replay_add

    def add(obs, act, rew, next_obs, done):
        rows.append(tuple(np.array(a, np.float32, copy=True) for a in (obs, act, rew, next_obs, done)))
        return real(obs, act, rew, next_obs, done)
    model.engine.replay_add = add
    return rows


@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("algo", ["dqn", "bdq"])
def test_parameters_equal_a_hand_driven_engine_fed_in_row_order(emulated_q_engine, algo, per):
    """Order pin: one replay_add of N rows per vectorised step, then the step's updates, then the target copy -- the same
    parameters, bit for bit, as an engine that receives the transitions one row at a time in env order and the train /
    train_per / update_target calls the rule yields."""
    env = DummyVecEnv([functools.partial(make_env, algo, k) for k in range(N_ENVS)])
    model = make_model(algo, env, per=per)
    rows = _spy_replay(model)
    model.learn(total_timesteps=TOTAL)
    assert len(rows) == TOTAL // N_ENVS and all(r[2].reshape(-1).shape[0] == N_ENVS for r in rows)
    hand = make_model(algo, DummyVecEnv([functools.partial(make_env, algo, k) for k in range(N_ENVS)]), per=per)
    eng = hand.engine
    beta = LinearSchedule(TOTAL, 1.0, hand.prioritized_replay_beta0)
    for (obs, act, rew, nxt, done), (n_upd, copy, ts) in zip(rows, expected_schedule(hand, N_ENVS, TOTAL, 64)):
        for i in range(N_ENVS):
            eng.replay_add(obs[i:i + 1], act.reshape(N_ENVS, -1)[i:i + 1], rew.reshape(-1)[i:i + 1], nxt[i:i + 1], done.reshape(-1)[i:i + 1])
        if n_upd and per:
            eng.train_per(n_upd, beta.value(ts))
        elif n_upd:
            eng.train(n_upd)
        if copy:
            eng.update_target()
    got, want = model.get_parameters(), eng.get_parameters()
    eps = [k for k in got if k.endswith("eps:0")][0]
    assert all(np.array_equal(got[k], want[k]) for k in got if k != eps)


@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("algo", ["dqn", "bdq"])
def test_one_environment_is_unchanged(emulated_q_engine, algo, per):
    """N = 1: the parameters after learn equal those of the loop that acted through `q_values(obs).argmax` on the host (the
    acting rule before the device-side arg-max, restated here by patching act_bins), and the exploration stream is consumed as
    that loop consumed it: one uniform per step and, only when it falls below epsilon, D bins."""
    def run(host_argmax):
        model = make_model(algo, DummyVecEnv([functools.partial(make_env, algo, 0)]), per=per)
        assert model.n_envs == 1 and model.engine.cfg.act_batch == 1
        if host_argmax:
            eng = model.engine
            eng.act_bins = lambda obs, explore=None: np.where(np.asarray(explore) >= 0, np.asarray(explore),
                                                              eng.q_values(np.asarray(obs, np.float32).reshape(1, -1)).argmax(axis=2))
        rows = _spy_replay(model)
        model.learn(total_timesteps=40)
        return model, rows
    new, rows_new = run(False)
    old, rows_old = run(True)
    assert new.n_updates == old.n_updates == 40 - 10
    for a, b in zip(rows_new, rows_old):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    pn, po = new.get_parameters(), old.get_parameters()
    assert all(np.array_equal(pn[k], po[k]) for k in pn)
    rng, sched = np.random.default_rng(3), new.exploration
    for t in range(40):
        if rng.random() < sched.value(t):
            rng.integers(0, new.bins, new.D)
    assert new._rng.bit_generator.state == rng.bit_generator.state == old._rng.bit_generator.state


@pytest.mark.parametrize("algo", ["dqn", "bdq"])
def test_ring_holds_the_transitions_the_environments_produced(emulated_q_engine, algo):
    """Row 4 k + i of the ring is environment i's transition of vectorised step k: observation, chosen bins, original reward,
    next observation AS THE VecEnv RETURNED IT (after an episode's end: the first observation of the next one) and done."""
    envs = [make_env(algo, k, cls=Recorder) for k in range(N_ENVS)]
    venv = DummyVecEnv([(lambda e=e: e) for e in envs])
    model = make_model(algo, venv, buffer_size=128)
    chosen = []
    real = model._act_bins
    model._act_bins = lambda obs, eps, always_draw=False: (chosen.append(real(obs, eps, always_draw)), chosen[-1])[1]
    model.learn(total_timesteps=TOTAL)
    steps = TOTAL // N_ENVS
    eng, B = model.engine, model.batch_size
    assert eng.replay_size() == TOTAL and any(d for e in envs for _, _, d in e.seen_steps)
    ends = [[k for k, s in enumerate(e.seen_steps) if s[2]] for e in envs]
    assert len({tuple(x) for x in ends}) == N_ENVS          # episodes ended at different steps in different rows
    for r0 in range(0, TOTAL, B):
        idx = np.arange(r0, r0 + B)
        eng.compute_grads(idx=idx)
        obs, nxt = eng.fetch("feat_pi", (B, OBS_DIM)), eng.fetch("feat_tgt", (B, OBS_DIM))
        act, rew, done = eng.fetch("act", (B, model.D)), eng.fetch("rew", (B,)), eng.fetch("done", (B,))
        for j, r in enumerate(idx):
            k, i = divmod(int(r), N_ENVS)
            e = envs[i]
            # what the VecEnv handed out: an env that finished was reset at once, its reset observation follows the terminal
            # one in seen_obs -- the observation of step k is the last one seen before step k, the next one the last after it
            n_resets = sum(1 for s in e.seen_steps[:k] if s[2])
            assert np.array_equal(obs[j], e.seen_obs[k + n_resets])
            assert np.array_equal(nxt[j], e.seen_obs[k + 1 + n_resets + (1 if e.seen_steps[k][2] else 0)])
            assert np.array_equal(act[j], chosen[k][i].astype(np.float32))
            assert rew[j] == np.float32(e.seen_steps[k][1]) and done[j] == float(e.seen_steps[k][2])
            env_action = np.asarray(model._bins_to_env_action(chosen[k][i]), np.float32).reshape(-1)
            assert np.array_equal(env_action, e.seen_steps[k][0].reshape(-1))
    assert len(chosen) == steps


@pytest.mark.parametrize("algo", ["dqn", "bdq"])
def test_predict_on_seven_rows_equals_seven_predictions(emulated_q_engine, algo):
    model = make_model(algo, DummyVecEnv([functools.partial(make_env, algo, k) for k in range(N_ENVS)]))
    model.learn(total_timesteps=48)
    obs = np.random.default_rng(5).uniform(-1, 1, (7, OBS_DIM)).astype(np.float32)
    batch, _ = model.predict(obs, deterministic=True)
    assert batch.shape[0] == 7
    singles = [model.predict(o, deterministic=True)[0] for o in obs]
    assert all(np.array_equal(batch[i], singles[i]) for i in range(7))
    q = np.concatenate([model.engine.q_values(obs[k:k + 4]) for k in (0, 4)])
    assert np.array_equal(np.asarray([model._bins_to_env_action(b) for b in q.argmax(axis=2)]), batch)
