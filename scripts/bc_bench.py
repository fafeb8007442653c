#!/usr/bin/env python
"""Updates per second of behaviour-cloning pretraining (grl_bc_train, csrc/plan_bc.inl) on three configurations -- the MLP policy
with layers [64, 64] and [128, 128] at 64 rows per minibatch on 101-value observations, and the depth `augmented` network at 256
rows -- development / documentation aid, not the headline bench.

    python scripts/bc_bench.py [--blocks 5] [--updates 64]

How it measures: a table of 2048 recorded rows is uploaded once; one timed unit is ONE grl_bc_train call of `--updates`
updates (one index row each, as an epoch of SAC.pretrain hands them over) followed by a synchronisation, so the call's index
check -- a copy of the indices to the host in front of the first launch -- and the host latency of its graph launches are
inside.  A block is as many units as fill at least 50 ms (asserted), sized from warmed units; the first block warms up and
captures the graphs; the figure is the median of the blocks with their spread.  The launch count per update comes from a
separate profiled call (grl_profile_dump: eager launches between events).
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

CONFIGS = {
    "mlp_64_64_b64": dict(extractor="mlp", obs_dim=101, layers=(64, 64), batch=64),
    "mlp_128_128_b64": dict(extractor="mlp", obs_dim=101, layers=(128, 128), batch=64),
    "depth_augmented_b256": dict(extractor="augmented", obs_channels=2, n_direct=1, layers=(64, 64), batch=256),
}
N_ROWS = 2048


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


def run(name, n_updates, n_blocks):
    from grasp_rl import _capi
    from grasp_rl.engine import SacEngine
    from grasp_rl.init import init_parameters
    c = dict(CONFIGS[name])
    batch = c.pop("batch")
    cfg = _capi.make_config(c.pop("extractor"), act_dim=5, batch_size=batch, replay_capacity=64, normalize=False, **c)
    eng = SacEngine(cfg)
    eng.set_parameters(init_parameters(eng.table, seed=0))
    rng = np.random.default_rng(0)
    obs = rng.normal(0, 1, (N_ROWS, 101)).astype(np.float32) if cfg.extractor == 0 else \
        rng.integers(0, 256, (N_ROWS, 64, 64, 2)).astype(np.float32)
    act = rng.uniform(-1, 1, (N_ROWS, 5)).astype(np.float32)
    eng.bc_begin(batch, 1e-4, 1e-8, -np.ones(5), np.ones(5))
    table = eng.bc_upload(obs, act)
    idx = np.stack([rng.permutation(N_ROWS)[:batch] for _ in range(n_updates)]).astype(np.int32)

    def unit():
        eng.bc_train(table, idx)
        eng.synchronize()
    med, lo, hi, k = _blocks(unit, n_blocks)
    eng.profile(True)
    eng.bc_train(table, idx[:1])
    eng.synchronize()
    prof = eng.profile_dump()
    eng.profile(False)
    eng.bc_end()
    eng.close()
    return {"what": "bc_train", "config": name, "bc_batch": batch, "updates_per_call": n_updates, "calls_per_block": k,
            "updates_per_s": round(n_updates / med, 1), "updates_per_s_min": round(n_updates / hi, 1), "updates_per_s_max": round(n_updates / lo, 1),
            "us_per_update": round(1e6 * med / n_updates, 2), "launches_per_update": int(sum(v["launches"] for v in prof.values())),
            "launch_us": {key: [int(v["launches"]), round(1e3 * v["avg_ms"] * v["launches"], 1)] for key, v in sorted(prof.items())}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--updates", type=int, default=64)
    ap.add_argument("--configs", nargs="+", default=sorted(CONFIGS))
    a = ap.parse_args()
    for name in a.configs:
        print(json.dumps(run(name, a.updates, a.blocks)), flush=True)
