#!/usr/bin/env python
"""Time of one TRPO update (grl_trpo_update: the natural-gradient policy step + the value fit, csrc/plan_trpo.inl) on the shapes
of config/simplified_object_picking.yaml -- observation 101, 5 actions, towers 64-64 -- at T = 400 (the reference's max_iters) and
T = 1024 (stable-baselines' default), and, for scale, the PPO2 update of the same towers per row processed -- development /
documentation aid, not the headline bench.

    python scripts/trpo_bench.py [--T 400 1024] [--blocks 5]

How it measures: a rollout is placed once; every update is re-armed through the "ppo_slots" debug word (which synchronises), so
one timed unit is `re-arm + update + synchronise` and the host-to-device latency of one graph launch is inside it.  A block is
as many units as fill at least 50 ms, the parameters are reset before every block (the launch list has a fixed shape, so the time
does not depend on them), the first block warms up and captures the graphs, and the figure is the median of the blocks with
their spread.  The per-launch table comes from a separate profiled update (grl_profile_dump: eager launches between events).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-rl-grasping_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np


def _rollout(rng, T, od, A):
    return dict(obs=rng.normal(0, 1, (1, T, od)).astype(np.float32), act=rng.normal(0, 1, (1, T, A)).astype(np.float32),
                val=rng.normal(0, 1, (1, T)).astype(np.float32), nlp=rng.normal(5, 1, (1, T)).astype(np.float32),
                rew=rng.normal(0, 1, (1, T)).astype(np.float32), done=(rng.random((1, T)) < 0.05).astype(np.float32))


def _blocks(unit, reset, n_blocks):
    """Median and spread of the time of `unit()` over blocks of >= 50 ms."""
    reset()
    for _ in range(3):      # warm-up: code objects, graph capture
        unit()
    t0 = time.perf_counter()
    for _ in range(5):      # the size of a block comes from warmed units
        unit()
    per = max((time.perf_counter() - t0) / 5, 1e-6)
    k = max(5, int(0.06 / per) + 1)
    out = []
    for _ in range(n_blocks + 1):
        reset()
        t0 = time.perf_counter()
        for _ in range(k):
            unit()
        out.append((time.perf_counter() - t0) / k)
    out = sorted(out[1:])
    assert k * out[0] >= 0.05, "a block shorter than 50 ms"
    return out[len(out) // 2], out[0], out[-1], k


def run_trpo(T, n_blocks, od=101, A=5):
    from grasp_rl import _capi
    from grasp_rl.engine import TrpoEngine
    from grasp_rl.init import init_ppo_parameters
    cfg, t = _capi.make_trpo_config(od, A, timesteps_per_batch=T)
    eng = TrpoEngine(cfg, t)
    P = init_ppo_parameters(eng.table, 0)
    rng = np.random.default_rng(0)
    r = _rollout(rng, T, od, A)
    eng.set_parameters(P)
    # actions the policy itself would have drawn, so that the surrogate and the line search see a realistic ratio
    r["act"] = np.stack([eng.act(r["obs"][0, k], deterministic=False) for k in range(T)], axis=1).reshape(1, T, A)
    eng.place_rollout(r["obs"], r["act"], r["val"], r["nlp"], r["rew"], r["done"])
    eng.finish(rng.normal(0, 1, od).astype(np.float32), [0.0])
    perm = np.stack([np.random.RandomState(k).permutation(T) for k in range(3)]).astype(np.int32)

    def unit():
        eng.store("ppo_slots", [T, T, 1])
        eng.update(perm)
        eng.synchronize()
    med, lo, hi, k = _blocks(unit, lambda: eng.set_parameters(P), n_blocks)
    m = eng.metrics()
    eng.set_parameters(P)
    eng.profile(True)
    unit()
    prof = eng.profile_dump()
    eng.profile(False)
    eng.close()
    return {"what": "trpo_update", "T": T, "obs_dim": od, "towers": [64, 64], "us_per_update": round(1e6 * med, 1), "us_min": round(1e6 * lo, 1),
            "us_max": round(1e6 * hi, 1), "updates_per_block": k, "us_per_row": round(1e6 * med / T, 3), "ls_index": m["ls_index"],
            "cg_iters": m["cg_iters"], "launches": int(sum(v["launches"] for v in prof.values())),
            "launch_us": {key: [int(v["launches"]), round(1e3 * v["avg_ms"] * v["launches"], 1)] for key, v in sorted(prof.items())}}


def run_ppo(T, n_blocks, od=101, A=5):
    """The PPO2 update of the same towers: 4 epochs x 4 minibatches over the same T rows (its defaults)."""
    from grasp_rl import _capi
    from grasp_rl.engine import PpoEngine
    from grasp_rl.init import init_ppo_parameters
    cfg, ppo = _capi.make_ppo_config(od, A, n_envs=1, n_steps=T, nminibatches=4)
    eng = PpoEngine(cfg, ppo)
    P = init_ppo_parameters(eng.table, 0)
    rng = np.random.default_rng(0)
    r = _rollout(rng, T, od, A)
    eng.set_parameters(P)
    eng.place_rollout(r["obs"], r["act"], r["val"], r["nlp"], r["rew"], r["done"])
    eng.finish(rng.normal(0, 1, (1, od)).astype(np.float32), [0.0])
    perm = np.stack([np.random.RandomState(k).permutation(T) for k in range(4)]).astype(np.int32)

    def unit():
        eng.store("ppo_slots", [T, T, 1])
        eng.train(perm)
        eng.synchronize()
    med, lo, hi, k = _blocks(unit, lambda: eng.set_parameters(P), n_blocks)
    eng.close()
    return {"what": "ppo2_train_4x4", "T": T, "us_per_call": round(1e6 * med, 1), "us_min": round(1e6 * lo, 1), "us_max": round(1e6 * hi, 1),
            "calls_per_block": k, "us_per_row_processed": round(1e6 * med / (4 * T), 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, nargs="+", default=[400, 1024])
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    for T in a.T:
        print(json.dumps(run_trpo(T, a.blocks)), flush=True)
        print(json.dumps(run_ppo(T, a.blocks)), flush=True)
