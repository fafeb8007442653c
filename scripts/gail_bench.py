#!/usr/bin/env python
"""Time of the two passes a GAIL session adds to a TRPO handle (grl_gail_rewards, grl_gail_update; csrc/plan_gail.inl) at the
shipped TRPO section -- T = 1024, towers 64-64, discriminator hidden 100, d_step = 1 (one update of 1024 + 1024 rows) -- on vector
observations (101 values) and on the 64 x 64 x 2 image flattened to 8192 values, with the TRPO update of the same handle beside
them for scale -- development / documentation aid, not the headline bench.

    python scripts/gail_bench.py [--blocks 5] [--configs vector image]

How it measures: a rollout of T rows is placed on the device and finished once; a timed unit is ONE call followed by a
synchronisation (grl_gail_update: one update, its index check -- a copy of the indices to the host -- inside; grl_gail_rewards:
the rollout is marked "full, not finished" again in front of every call, outside the timed span; grl_trpo_update: the rollout is
marked finished again in front of every call, 3 value-fit permutations).  A block is as many units as fill at least 50 ms
(asserted), sized from warmed units; the first block warms up and captures the graphs; the figure is the median of the blocks
with their spread.  Launch counts come from the plan dump (GRL_PLAN_DUMP)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-rl-grasping_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

CONFIGS = {"vector": 101, "image": 8192}
T, A, HIDDEN, N_ROWS = 1024, 5, 100, 2048


def _blocks(unit, before, n_blocks):
    def timed():
        before()
        t0 = time.perf_counter()
        unit()
        return time.perf_counter() - t0
    for _ in range(3):      # warm-up: code objects, graph capture
        timed()
    per = max(sum(timed() for _ in range(3)) / 3, 1e-6)
    k = max(2, int(0.06 / per) + 1)
    out = []
    for _ in range(n_blocks + 1):
        out.append(sum(timed() for _ in range(k)) / k)
    out = sorted(out[1:])
    assert k * out[0] >= 0.05, "a block shorter than 50 ms"
    return {"us": round(1e6 * out[len(out) // 2], 1), "us_min": round(1e6 * out[0], 1), "us_max": round(1e6 * out[-1], 1), "units_per_block": k}


def run(name, n_blocks):
    from grasp_rl import _capi
    from grasp_rl.engine import TrpoEngine
    from grasp_rl.init import init_ppo_parameters
    od = CONFIGS[name]
    cfg, trpo = _capi.make_trpo_config(od, A, timesteps_per_batch=T)
    eng = TrpoEngine(cfg, trpo)
    eng.set_parameters(init_ppo_parameters(eng.table, 0))
    rng = np.random.default_rng(0)
    z = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    es = (rng.random(T) < 0.1).astype(np.float32)
    eng.place_rollout(z(1, T, od), z(1, T, A), z(1, T), z(1, T) + 5.0, z(1, T), es[None])
    eng.finish(z(od), [0.0])
    eng.gail_begin(HIDDEN, T, 1e-3, 3e-4, -np.ones(A), np.ones(A))
    shapes = eng.gail_param_shapes()
    eng.gail_set_parameters({n: (rng.uniform(-1, 1, s) * np.sqrt(6.0 / sum(s))).astype(np.float32) if len(s) == 2 else np.zeros(s, np.float32)
                             for n, s in shapes.items()})
    table = eng.gail_upload(z(N_ROWS, od), rng.uniform(-1, 1, (N_ROWS, A)).astype(np.float32))
    gen = rng.permutation(T).astype(np.int32)[None]
    exp = rng.permutation(N_ROWS)[:T].astype(np.int32)[None]
    vf_perm = np.stack([rng.permutation(T) for _ in range(3)]).astype(np.int32)
    sync = eng.synchronize
    res = {"what": "gail", "config": name, "obs_dim": od, "T": T, "hidden": HIDDEN}
    res["gail_update"] = _blocks(lambda: (eng.gail_update(table, gen, exp), sync()), lambda: None, n_blocks)
    res["gail_rewards"] = _blocks(lambda: (eng.gail_rewards(), sync()), lambda: eng.store("ppo_slots", [T, T, 0]), n_blocks)
    res["trpo_update"] = _blocks(lambda: (eng.update(vf_perm), sync()), lambda: eng.store("ppo_slots", [T, T, 1]), n_blocks)
    eng.gail_end()
    eng.close()
    return res


def plan_lines(name):
    """the two `grl plan: gail ...` lines of the configuration, from a child process that only sizes the session"""
    code = ("import sys; sys.path[:0] = %r; import numpy as np; from grasp_rl import _capi; from grasp_rl.engine import TrpoEngine; "
            "cfg, t = _capi.make_trpo_config(%d, %d, timesteps_per_batch=%d); e = TrpoEngine(cfg, t); "
            "e.gail_begin(%d, %d, 1e-3, 3e-4, -np.ones(%d), np.ones(%d)); e.gail_end(); e.close()"
            % ([ROOT, os.path.join(ROOT, "deep-rl-grasping_amd")], CONFIGS[name], A, T, HIDDEN, T, A, A))
    err = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GRL_PLAN_DUMP="1"), stderr=subprocess.PIPE, check=True).stderr.decode()
    return {k: {"launches": int(n), "first_layer": r}
            for k, n, r in set(re.findall(r"grl plan: gail (rewards|update) +(\d+) launches.*first layer (whole|split \d+)", err))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--configs", nargs="+", default=sorted(CONFIGS))
    a = ap.parse_args()
    for name in a.configs:
        out = run(name, a.blocks)
        out["plan"] = plan_lines(name)
        print(json.dumps(out), flush=True)
