#!/usr/bin/env python
"""SAC CnnPolicy on square depth images of another size than 64x64 (grl_config.img_hw 36 .. 128): updates/s and the
per-launch table on one GPU, batch 256, layers [64, 64].  These sizes run the per-layer implicit-GEMM route (conv_stack.h is
64x64 only), so the headline figure of bench.py is not their yardstick.  Development / documentation aid; bench.py stays as it is.

    python scripts/sac_image_size_bench.py --hw 84 [--batch 256] [--replay 4096] [--steps 300] [--repeats 3]
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
import torch

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=84)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--replay", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    from grasp_rl import _capi, synthetic
    from grasp_rl.engine import SacEngine
    from grasp_rl.init import init_parameters
    dev = torch.device("cuda", 0)
    cfg = _capi.make_config("augmented", obs_channels=2, n_direct=1, act_dim=5, layers=(64, 64), batch_size=a.batch,
                            replay_capacity=a.replay, normalize=True, act_batch=16, seed=1, img_hw=a.hw)
    t0 = time.perf_counter()
    eng = SacEngine(cfg, device=str(dev))
    t_create = time.perf_counter() - t0
    eng.set_parameters(init_parameters(eng.table, seed=0))
    st = synthetic.load_obs_stats("depth")
    ii = (np.arange(a.hw) * 64) // a.hw                  # the shipped 64x64 statistics, nearest pixel
    mean_h, var_h = st["mean"][ii][:, ii], st["var"][ii][:, ii]
    mean = torch.from_numpy(np.ascontiguousarray(mean_h, np.float32)).to(dev)
    std = torch.from_numpy(np.sqrt(var_h).astype(np.float32)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    for k0 in range(0, a.replay, 1024):
        m = min(1024, a.replay - k0)
        with torch.cuda.stream(eng.be.stream):
            def draw():
                o = mean + std * torch.randn((m,) + tuple(mean.shape), generator=g, device=dev)
                o[..., 0].clamp_(0.02, 2.0)
                o[..., 1] = 0.0
                o[:, 0, 0, 1] = torch.rand(m, generator=g, device=dev)
                return o.contiguous()
            eng.replay_add_device(draw(), (torch.rand((m, 5), generator=g, device=dev) * 2 - 1).contiguous(),
                                  torch.randn(m, generator=g, device=dev).contiguous(), draw(),
                                  (torch.rand(m, generator=g, device=dev) < 1 / 15).float().contiguous())
        eng.be.stream.synchronize()
    eng.set_obs_stats(mean_h, var_h, st["ret_var"])
    eng.train_device(30)
    eng.synchronize()
    rates = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        eng.train_device(a.steps)
        eng.synchronize()
        rates.append(a.steps / (time.perf_counter() - t0))
    eng.profile(True)
    eng.train_device(30)
    eng.synchronize()
    prof = eng.profile_dump()
    m = eng.metrics()
    print(json.dumps({"workload": "SAC depth %dx%dx2, batch %d" % (a.hw, a.hw, a.batch), "updates_per_s": [round(r, 1) for r in rates],
                      "median": round(float(np.median(rates)), 1), "spread": round(max(rates) - min(rates), 1),
                      "create_s": round(t_create, 2), "finite": bool(np.isfinite([m[k] for k in m]).all()),
                      "launch_us": {k: round(1e3 * v["avg_ms"] * v["launches"] / 30.0, 1) for k, v in sorted(prof.items())}}))
    eng.close()
