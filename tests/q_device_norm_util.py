"""Shared bodies of the "VecNormalize statistics and observe-once on DQN / BDQ handles" checks: run on the emulation build by
tests/test_hostemu_q_device_norm.py and on the MI355X by tests/test_gpu_q_device_norm.py.  make_engine(cfg) builds a QEngine;
every comparison is exact (raw words where floats are compared).

The calls are the ones include/grl.h documents for SAC handles (grl_norm_update, grl_observe, grl_replay_add_observed,
grl_act with GRL_ACT_RAW_OBS / GRL_ACT_OBSERVED); on a Q handle they combine with GRL_ACT_GREEDY.  What the device computes must
be what the separate host steps compute: RunningMeanStd.update for the statistics, VecNormalize.normalize_obs in front of the
plain greedy act, grl_replay_add for the ring, grl_set_obs_stats in front of an update."""
import ctypes as C

import numpy as np

from grasp_rl import _capi
from grasp_rl.sb.running_mean_std import RunningMeanStd
from grasp_rl.sb.vec_env import VecNormalize

ERR_INVALID, ERR_STATE = -1, -3
ACT_BATCH = 64
ROWS = (1, 16, 17, 64)            # one row; one full row block of q_act.h; a second, ragged one; four
# the two reference networks (DQN 5 bins [64, 64]; BDQ [[64, 64], [32], [32]], 3 x 33 bins) at the observation widths on both sides of the one-launch kernel's limit (128), and one network with a
# width past its 64-wide stages; `fused`: the route the case exists for (csrc/q_act.h qa_shape_ok), asserted from the plan dump
NETS = {"dqn": dict(algo="dqn", D=1, bins=5, common=(), branch=(64, 64), value=(64, 64)),
        "bdq": dict(algo="bdq", D=3, bins=33, common=(64, 64), branch=(32,), value=(32,)),
        "bdq_w65": dict(algo="bdq", D=3, bins=33, common=(64, 65), branch=(32,), value=(32,))}
ACT_CASES = [("dqn", 1, True), ("dqn", 100, True), ("dqn", 128, True), ("dqn", 129, False),
             ("bdq", 1, True), ("bdq", 100, True), ("bdq", 128, True), ("bdq", 129, False), ("bdq_w65", 100, False)]


def q_cfg(net, obs_dim, batch_size=8, capacity=64, **kw):
    a = NETS[net]
    return _capi.make_q_config(a["algo"], obs_dim, a["D"], a["bins"], a["common"], a["branch"], a["value"], batch_size=batch_size,
                               act_batch=ACT_BATCH, replay_capacity=capacity, normalize=True, clip_obs=10.0, **kw)


def init_params(eng, seed=11):
    """Xavier-uniform kernels, biases away from zero (every bias add and the value tower take part), target = online."""
    rng = np.random.default_rng(seed)
    P = {}
    for name, _, _, shape, _ in eng.table:
        if "/target_q_func/" in name:
            continue
        if name.endswith("weights:0"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            P[name] = rng.uniform(-lim, lim, shape).astype(np.float32)
        elif name.endswith("eps:0"):
            P[name] = np.float32(0.1).reshape(())
        else:
            P[name] = rng.uniform(-0.1, 0.1, shape).astype(np.float32)
    for name, *_ in eng.table:
        if "/target_q_func/" in name:
            P[name] = P[name.replace("/target_q_func", "")].copy()
    eng.set_parameters(P)
    return P


def raw_batches(rng, obs_dim, sizes=ROWS):
    """float32 batches of raw observations: column 0 constant, values of 1e4 in the last column (and in rows of the others)."""
    out = []
    for k, n in enumerate(sizes):
        x = (rng.normal(0.5, 2.0, (n, obs_dim)) * (1.0 + np.arange(obs_dim) % 3)).astype(np.float32)
        x[:, 0] = 3.25
        if obs_dim > 1:
            x[:, -1] = 1e4 + k
            x[n // 2, 1:] += np.float32(1e4)
        out.append(x)
    return out


def words(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def expect_error(eng, code, call):
    """`call()` is a raw library call: its return code and a non-empty grl_last_error."""
    rc = call()
    assert rc == code, (rc, code)
    assert eng.lib.grl_last_error().decode().strip(), "grl_last_error is empty"


def host_normalize(mean, var, obs, clip_obs=10.0, eps=1e-8):
    """VecNormalize.normalize_obs itself, on the given statistics, cast to float32."""
    vn = VecNormalize.__new__(VecNormalize)
    vn.norm_obs, vn.clip_obs, vn.epsilon = True, clip_obs, eps
    vn.obs_rms = RunningMeanStd(shape=mean.shape)
    vn.obs_rms.mean, vn.obs_rms.var = mean, var
    with np.errstate(invalid="ignore"):
        return np.asarray(vn.normalize_obs(obs), np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ 1. statistics
def check_statistics(make_engine, obs_dim=100):
    a, b = make_engine(q_cfg("bdq", obs_dim)), make_engine(q_cfg("bdq", obs_dim))
    try:
        ref = RunningMeanStd(shape=(obs_dim,))
        for e in (a, b):          # a new handle holds RunningMeanStd(): mean 0, var 1, count 1e-4
            m, v, c = e.get_obs_stats((obs_dim,))
            assert np.array_equal(m, ref.mean) and np.array_equal(v, ref.var) and c == ref.count
        batches = raw_batches(np.random.default_rng(5), obs_dim) + raw_batches(np.random.default_rng(6), obs_dim, ROWS[::-1])
        for k, x in enumerate(batches):
            ref.update(x)
            a.norm_update(x)
            b.observe(x, update_stats=True)
            for name, e in (("grl_norm_update", a), ("grl_observe", b)):
                m, v, c = e.get_obs_stats((obs_dim,))
                assert m.dtype == np.float64 and np.array_equal(words(m), words(np.asarray(ref.mean))), (name, k)
                assert np.array_equal(words(v), words(np.asarray(ref.var))), (name, k)
                assert np.float64(c).tobytes() == np.float64(ref.count).tobytes(), (name, k)
        b.observe(batches[0])                                   # without the flag: nothing moves
        m, v, c = b.get_obs_stats((obs_dim,))
        assert np.array_equal(words(m), words(np.asarray(ref.mean))) and c == ref.count
        # grl_set_running_stats: the starting point is taken as given
        a.set_running_stats(ref.mean * 0.5, ref.var * 2.0, 7.0)
        m, v, c = a.get_obs_stats((obs_dim,))
        assert np.array_equal(m, ref.mean * 0.5) and np.array_equal(v, ref.var * 2.0) and c == 7.0
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------ 2. act
def act_rows(rng, mean, var, n):
    """n raw rows around the statistics: values beyond clip_obs on both sides in every row block, row 1 all NaN."""
    sd = np.sqrt(var + 1e-8)
    x = (mean + sd * rng.normal(0.0, 1.5, (n, mean.shape[0]))).astype(np.float32)
    x[0, 0] = np.float32(mean[0] + 50.0 * sd[0] + 1.0)
    x[n - 1, -1] = np.float32(mean[-1] - 50.0 * sd[-1] - 1.0)
    x[n // 2, :] = (mean + 30.0 * sd * np.where(np.arange(mean.shape[0]) % 2, 1.0, -1.0) + 1.0).astype(np.float32)
    if n > 1:
        x[1, :] = np.nan
    return x


def check_act(make_engine, read_plan, net, obs_dim, fused):
    eng = make_engine(q_cfg(net, obs_dim))
    try:
        plan = read_plan()
        assert ("epsilon-greedy act: one launch" in plan) == fused and ("+ select kernel" in plan) != fused, plan
        init_params(eng)
        D, bins = eng.D, eng.bins
        rng = np.random.default_rng(17)
        for x in raw_batches(rng, obs_dim):
            eng.norm_update(x)
        mean, var, _ = eng.get_obs_stats((obs_dim,))
        differ = 0
        for n in ROWS:
            sets = [act_rows(rng, mean, var, n)]
            if n == 1:
                sets.append(np.full((1, obs_dim), np.nan, np.float32))      # the all-NaN row as the only row
            for raw in sets:
                norm = host_normalize(mean, var, raw)
                finite = ~np.isnan(raw).any(axis=1)
                if n > 1:          # clipped on both sides
                    assert (norm[finite] == 10.0).any() and (norm[finite] == -10.0).any()
                explore = np.where(rng.random((n, D)) < 0.5, rng.integers(0, bins, (n, D)), -1)
                explore[0, 0] = -1 if n > 1 else explore[0, 0]
                if n > 1:
                    explore[n - 1] = np.arange(D) % bins
                for table in (explore, None):
                    want = eng.act_bins(norm, table)                         # plain GRL_ACT_GREEDY on the host's normalize_obs
                    got = eng.act_bins(raw, table, raw=True)
                    assert np.array_equal(got, want), ("RAW_OBS", n, np.argwhere(got != want)[:4])
                    eng.observe(raw)
                    got = eng.act_bins(n, table, raw=True, observed=True)
                    assert np.array_equal(got, want), ("OBSERVED | RAW_OBS", n, np.argwhere(got != want)[:4])
                    eng.observe(norm)
                    got = eng.act_bins(n, table, observed=True)
                    assert np.array_equal(got, want), ("OBSERVED", n, np.argwhere(got != want)[:4])
                    if table is None and n > 1:
                        differ += int((want != eng.act_bins(np.nan_to_num(raw, nan=0.0), None)).any())
        assert differ > 0          # the greedy bins do depend on the normalisation (raw rows handed over as normalised ones differ)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ 3. replay rows
def replay_words(eng):
    """The words of every array grl_replay_segments lists, one after the other."""
    flat = np.ascontiguousarray(eng.be.to_host(eng.replay)).view(np.uint32)
    size, out = eng.replay_size(), []
    segs = eng.replay_segments()
    for seg in segs:
        lo, hi = eng._segment_span(seg, size)
        out.append(flat[lo:hi].copy())
    return segs, out


def check_replay_rows(make_engine, net="bdq", obs_dim=100, n=16, steps=3):
    cfg = lambda: q_cfg(net, obs_dim, capacity=40, prioritized=True)
    a, b = make_engine(cfg()), make_engine(cfg())
    try:
        D, bins = a.D, a.bins
        rng = np.random.default_rng(23)
        obs = raw_batches(rng, obs_dim, (n,))[0]
        b.observe(obs, update_stats=True)
        for step in range(steps):
            act = rng.integers(0, bins, (n, D)).astype(np.float32)
            rew = rng.normal(size=n).astype(np.float32)
            done = np.zeros(n, np.float32)
            new = raw_batches(rng, obs_dim, (n,))[0]
            rows, term = [], None
            if step == 1:                               # two terminal rows: their terminal observations are stored as `next`
                rows = [3, 12]
                done[rows] = 1.0
                term = raw_batches(rng, obs_dim, (2,))[0]
            store = new.copy()
            for j, i in enumerate(rows):
                store[i] = term[j]
            a.replay_add(obs, act, rew, store, done)
            b.observe(new, update_stats=True)
            b.replay_add_observed(act, rew, done, rows, term)
            assert a.replay_size() == b.replay_size() == min(40, n * (step + 1))
            obs = new
        (sa, wa), (sb, wb) = replay_words(a), replay_words(b)
        assert sa == sb and len(sa) == 5 + 4           # obs, next, act, rew, done + priority leaves, block sums, minima, state
        for k, (x, y) in enumerate(zip(wa, wb)):
            assert x.shape == y.shape and x.size and np.array_equal(x, y), "segment %d differs in %d words" % (k, int((x != y).sum()))
        assert np.array_equal(a.stored_priorities(), b.stored_priorities()) and a.stored_priorities().all()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------ 4. updates
def check_updates(make_engine, net="bdq", obs_dim=100, B=8, n_store=48):
    cfg = lambda: q_cfg(net, obs_dim, batch_size=B, capacity=64, prioritized=True)
    a, b = make_engine(cfg()), make_engine(cfg())
    try:
        P = init_params(a)
        b.set_parameters(P)
        D, bins = a.D, a.bins
        rng = np.random.default_rng(29)
        tr = dict(obs=raw_batches(rng, obs_dim, (n_store,))[0], nxt=raw_batches(rng, obs_dim, (n_store,))[0],
                  act=rng.integers(0, bins, (n_store, D)).astype(np.float32), rew=rng.normal(0, 2, n_store).astype(np.float32),
                  done=(rng.random(n_store) < 0.2).astype(np.float32))
        for e in (a, b):
            e.replay_add(tr["obs"], tr["act"], tr["rew"], tr["nxt"], tr["done"])
        ref = RunningMeanStd(shape=(obs_dim,))

        def step_statistics(k):
            """one env step's worth of observations: the host folds them in and pushes (A), the device folds them in (B)"""
            x = raw_batches(rng, obs_dim, (ROWS[k % len(ROWS)],))[0]
            ref.update(x)
            ret_var = 4.0 + k
            a.set_obs_stats(ref.mean, ref.var, ret_var)
            b.norm_update(x)
            b.set_ret_var(ret_var)

        for k in range(3):
            step_statistics(k)
            idx = rng.integers(0, n_store, (1, B), dtype=np.int64)
            w = rng.uniform(0.3, 1.0, (1, B)).astype(np.float32)
            a.train(1, idx, w)
            b.train(1, idx, w)
        step_statistics(3)
        u = rng.random((1, B))
        a.train_per(1, 0.6, u)
        b.train_per(1, 0.6, u)
        Pa, Pb = a.get_parameters(), b.get_parameters()
        moved = 0
        for name in Pa:
            assert np.array_equal(words(Pa[name]), words(Pb[name])), name
            moved += int(not np.array_equal(Pa[name], P[name]))
        assert moved > len(Pa) // 3
        assert np.array_equal(a.sampled_indices(), b.sampled_indices())
        assert np.array_equal(a.stored_priorities(), b.stored_priorities())
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------ 5. errors
def check_errors(make_engine, net="bdq", obs_dim=100, n=16):
    eng = make_engine(q_cfg(net, obs_dim))
    try:
        init_params(eng)
        lib, h, D, bins = eng.lib, eng.h, eng.D, eng.bins
        rng = np.random.default_rng(31)
        obs = raw_batches(rng, obs_dim, (n,))[0]
        out = np.empty((ACT_BATCH, D * bins), np.float32)
        act = np.zeros((n, D), np.float32)
        rew, done = np.zeros(n, np.float32), np.zeros(n, np.float32)
        p = lambda arr: arr.ctypes.data
        G, RAW, OBS = _capi.ACT_GREEDY, _capi.ACT_RAW_OBS, _capi.ACT_OBSERVED
        # nothing observed yet
        expect_error(eng, ERR_STATE, lambda: lib.grl_act(h, None, n, G | OBS, None, p(out)))
        expect_error(eng, ERR_STATE, lambda: lib.grl_replay_add_observed(h, p(act), p(rew), p(done), n, None, None, 0))
        eng.observe(obs)
        # OBSERVED with the wrong n; a replay row after a single grl_observe
        expect_error(eng, ERR_STATE, lambda: lib.grl_act(h, None, n - 1, G | OBS, None, p(out)))
        expect_error(eng, ERR_STATE, lambda: lib.grl_act(h, None, n + 1, G | OBS | RAW, None, p(out)))
        expect_error(eng, ERR_STATE, lambda: lib.grl_replay_add_observed(h, p(act), p(rew), p(done), n, None, None, 0))
        eng.observe(obs[:n - 1])
        expect_error(eng, ERR_STATE, lambda: lib.grl_replay_add_observed(h, p(act), p(rew), p(done), n, None, None, 0))
        # more rows than max(act_batch, 64)
        big = np.zeros((max(ACT_BATCH, 64) + 1, obs_dim), np.float32)
        expect_error(eng, ERR_INVALID, lambda: lib.grl_observe(h, p(big), big.shape[0], 0))
        expect_error(eng, ERR_INVALID, lambda: lib.grl_norm_update(h, p(big), big.shape[0]))
        # the Q-value form of grl_act keeps refusing both flags
        for flags in (RAW, OBS, RAW | OBS, 1 | RAW, 1 | OBS):
            expect_error(eng, ERR_STATE, lambda: lib.grl_act(h, p(obs), n - 1, flags, None, p(out)))
        assert eng.act_bins(n - 1, None, raw=True, observed=True).shape == (n - 1, D)      # the handle still works
        # a connected handle (world of one: the peer is the rank itself): the statistics calls say that they do not merge
        eng.allreduce_connect([eng.allreduce_init(0, 1)])
        try:
            expect_error(eng, ERR_STATE, lambda: lib.grl_norm_update(h, p(obs), n))
            assert "data-parallel" in lib.grl_last_error().decode()
            expect_error(eng, ERR_STATE, lambda: lib.grl_observe(h, p(obs), n, 1))
            assert "data-parallel" in lib.grl_last_error().decode()
            assert lib.grl_observe(h, p(obs), n, 0) == 0                                   # uploading alone is no merge
        finally:
            eng.allreduce_disconnect()
        eng.norm_update(obs)                                                                # single-process again
    finally:
        eng.close()
