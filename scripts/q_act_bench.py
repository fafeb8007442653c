"""Act latency of a DQN / BDQ handle and the BDQ learn-loop rate on N environments.

  python scripts/q_act_bench.py act   [--path q|greedy|observed|both] [--calls 2000]   # grl_act on the BDQ handle of
                                                  # config/gripper_grasp.yaml, n = 1, 16, 64: Q-value path / GRL_ACT_GREEDY path /
                                                  # GRL_ACT_GREEDY | RAW_OBS | OBSERVED on rows grl_observe uploaded (not in `both`)
  python scripts/q_act_bench.py learn [--envs 1] [--steps 20000] [--device-norm 0|1]   # BDQ.learn on grasp_rl.synthetic.ReachGraspEnv;
                                                  # --device-norm: BDQ(device_norm=...), statistics on the host / on the device

Prints one JSON line.  GRL_LIBRARY selects the library (an A/B against another build: alternate processes, one build each);
a library without GRL_ACT_GREEDY answers the `greedy` path with null.  Wall-clock per call, host side: the median of `calls`
calls after 200 warm-up calls."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-rl-grasping_amd"))


def bench_act(args):
    from grasp_rl import _capi
    from grasp_rl.engine import QEngine
    out = {"what": "grl_act on the BDQ handle (obs 101, 5 branches x 33 bins, [[64, 64], [32], [32]])", "calls": args.calls,
           "library": os.environ.get("GRL_LIBRARY", "in-tree")}
    rng = np.random.default_rng(0)
    for n in (1, 16, 64):
        cfg = _capi.make_q_config("bdq", 101, 5, 33, (64, 64), (32,), (32,), batch_size=64, act_batch=n, replay_capacity=1024)
        eng = QEngine(cfg)
        P = {name: rng.uniform(-0.1, 0.1, shape).astype(np.float32) for name, _, _, shape, _ in eng.table}
        eng.set_parameters(P)
        obs = rng.normal(0, 1, (n, 101)).astype(np.float32)
        explore = np.where(rng.random((n, 5)) < 0.1, rng.integers(0, 33, (n, 5)), -1)
        paths = {"q": lambda: eng.q_values(obs), "greedy": lambda: eng.act_bins(obs, explore),
                 "observed": lambda: eng.act_bins(n, explore, raw=True, observed=True)}
        for name in (("q", "greedy") if args.path == "both" else (args.path,)):
            f = paths[name]
            try:
                if name == "observed":
                    eng.set_obs_stats(np.zeros(101), np.ones(101), 1.0)
                    eng.observe(obs)
                for _ in range(200):
                    f()
            except (_capi.GrlError, TypeError):          # a build without the flag
                out["%s_n%d_us" % (name, n)] = None
                continue
            t = np.empty(args.calls)
            for k in range(args.calls):
                t0 = time.perf_counter()
                f()
                t[k] = time.perf_counter() - t0
            out["%s_n%d_us" % (name, n)] = round(float(np.median(t)) * 1e6, 2)
            out["%s_n%d_p10_p90_us" % (name, n)] = [round(float(np.percentile(t, p)) * 1e6, 2) for p in (10, 90)]
        eng.close()
    return out


def bench_learn(args):
    from grasp_rl import synthetic
    kw = {"q_envs": args.envs} if args.envs != 1 else {}      # (one environment: also runs on a tree without the fan-out)
    if args.device_norm is not None:                           # (unset: also runs on a tree without the option)
        kw["device_norm"] = bool(args.device_norm)
    r = synthetic.learn_reach("bdq", "vector", total_timesteps=args.steps, eval_episodes=20, **kw)
    return {"what": "BDQ.learn on ReachGraspEnv (prioritised replay, batch 64)", "envs": args.envs, "device_norm": args.device_norm,
            "env_steps": r["env_steps"],
            "updates": r["updates"], "seconds": r["seconds"], "env_steps_per_s": round(r["env_steps"] / r["seconds"], 1),
            "updates_per_s": round(r["updates"] / r["seconds"], 1)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["act", "learn"])
    ap.add_argument("--path", default="both", choices=["q", "greedy", "observed", "both"])
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--envs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--device-norm", type=int, default=None, choices=[0, 1])
    a = ap.parse_args()
    print(json.dumps(bench_act(a) if a.mode == "act" else bench_learn(a)))
