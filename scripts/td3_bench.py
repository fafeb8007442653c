#!/usr/bin/env python
"""Updates per second of TD3 (grl_td3_train, csrc/plan_td3.inl) at obs_dim 101, 5 action components, layers [64, 64],
policy_delay 2, at 64 and 256 rows per minibatch -- development / documentation aid, not the headline bench.

    python scripts/td3_bench.py [--blocks 5] [--updates 64] [--sac]

How it measures: the replay holds 4096 rows; one timed unit is ONE grl_td3_train call of `--updates` updates on the device draws
(half of them policy updates) followed by a synchronisation, so the host latency of its graph launches is inside.  A block is as
many units as fill at least 50 ms (asserted), sized from warmed units; the first block warms up and captures the graphs; the
figure is the median of the blocks with their spread.  The launch counts per update come from profiled calls of one update each
(grl_profile_dump: eager launches between events).  --sac: for orientation, a SAC-MLP handle of the same observation / layers /
batch through grl_train_step; run it with GRL_NO_FUSED_HEADS=1 for the per-layer route TD3's launch list is modelled on.
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

OBS, ACT, LAYERS, N_ROWS = 101, 5, (64, 64), 4096
BATCHES = (64, 256)


def _blocks(unit, n_blocks):
    for _ in range(3):      # warm-up: code objects, graph capture
        unit()
    t0 = time.perf_counter()
    for _ in range(3):      # the size of a block comes from warmed units
        unit()
    per = max((time.perf_counter() - t0) / 3, 1e-6)
    k = max(2, int(0.06 / per) + 1)
    out = []
    for _ in range(n_blocks + 1):
        t0 = time.perf_counter()
        for _ in range(k):
            unit()
        out.append((time.perf_counter() - t0) / k)
    out = sorted(out[1:])
    assert k * out[0] >= 0.05, "a block shorter than 50 ms"
    return out[len(out) // 2], out[0], out[-1], k


def _fill(eng):
    rng = np.random.default_rng(0)
    eng.replay_add(rng.normal(0, 1, (N_ROWS, OBS)).astype(np.float32), rng.uniform(-1, 1, (N_ROWS, ACT)).astype(np.float32),
                   rng.normal(0, 1, N_ROWS).astype(np.float32), rng.normal(0, 1, (N_ROWS, OBS)).astype(np.float32),
                   (rng.random(N_ROWS) < 0.1).astype(np.float32))


def _launches(eng, train):
    eng.profile(True)
    train()
    eng.synchronize()
    n = int(sum(v["launches"] for v in eng.profile_dump().values()))
    eng.profile(False)
    return n


def _row(what, batch, n_updates, med, lo, hi, k, extra):
    return dict({"what": what, "batch": batch, "updates_per_call": n_updates, "calls_per_block": k,
                 "updates_per_s": round(n_updates / med, 1), "updates_per_s_min": round(n_updates / hi, 1),
                 "updates_per_s_max": round(n_updates / lo, 1), "us_per_update": round(1e6 * med / n_updates, 2)}, **extra)


def run_td3(batch, n_updates, n_blocks):
    from grasp_rl import _capi
    from grasp_rl.engine import Td3Engine
    from grasp_rl.init import init_parameters
    cfg, td3 = _capi.make_td3_config(OBS, ACT, layers=LAYERS, batch_size=batch, replay_capacity=N_ROWS, policy_delay=2)
    eng = Td3Engine(cfg, td3)
    eng.set_parameters(init_parameters(eng.table, seed=0))
    _fill(eng)

    def unit():
        eng.train(n_updates, first_step=0)
        eng.synchronize()
    med, lo, hi, k = _blocks(unit, n_blocks)
    extra = {"launches_critic_only": _launches(eng, lambda: eng.train(1, first_step=1)),
             "launches_policy_update": _launches(eng, lambda: eng.train(1, first_step=0)), "policy_delay": 2}
    eng.close()
    return _row("td3_train", batch, n_updates, med, lo, hi, k, extra)


def run_sac(batch, n_updates, n_blocks):
    from grasp_rl import _capi
    from grasp_rl.engine import SacEngine
    from grasp_rl.init import init_parameters
    cfg = _capi.make_config("mlp", obs_dim=OBS, act_dim=ACT, layers=LAYERS, batch_size=batch, replay_capacity=N_ROWS, normalize=False)
    eng = SacEngine(cfg)
    eng.set_parameters(init_parameters(eng.table, seed=0))
    _fill(eng)

    def unit():
        eng.train(n_updates)
        eng.synchronize()
    med, lo, hi, k = _blocks(unit, n_blocks)
    extra = {"launches_per_update": _launches(eng, lambda: eng.train(1)), "GRL_NO_FUSED_HEADS": os.environ.get("GRL_NO_FUSED_HEADS", "")}
    eng.close()
    return _row("sac_mlp_train_step", batch, n_updates, med, lo, hi, k, extra)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--updates", type=int, default=64)
    ap.add_argument("--sac", action="store_true")
    a = ap.parse_args()
    for batch in BATCHES:
        print(json.dumps((run_sac if a.sac else run_td3)(batch, a.updates, a.blocks)), flush=True)
