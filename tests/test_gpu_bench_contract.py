"""The line `bench.py` prints is what the driver reads: one JSON object with the contract's keys, the BASELINE metric and
workload; with --full also a `roofline` whose numbers follow from each other, and a `cpu_baseline` from the oracle (the only
place outside tests/ and smoke() where oracle/ runs -- never inside the timed region).  A plain run times exactly --steps
updates and does nothing else; --dump-outputs writes what the timed path computed, the same in every run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=e, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, "exactly one line on stdout"
    return json.loads(lines[0])


def test_bench_line_contract():
    d = _bench("--gpus", "1", "--steps", "40", "--warmup", "5", "--full", "--no-learn-loop", "--no-success")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["n_gpus"] == 1 and d["steps"] == 40 and d["warmup"] == 5 and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None and d["scaling"] == "weak"
    assert "grad-steps" in d["metric"] and "grad-steps" in json.dumps(base)      # BASELINE.json's metric
    assert "workload" in d["config"] and "batch 256" in d["config"]["workload"] and "model" not in d["config"]
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 0.01                 # value = steps / time
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 157.3
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert abs(r["achieved"] - r["flops_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12) < 0.05 * r["achieved"]
    assert abs(r["step_frac"] - r["step_flops"] / (d["ms_per_step"] * 1e-3) / 1e12 / r["peak"]) < 2e-3
    assert r["step_flops"] <= r["step_flops_executed"] * (1 + 1e-9)
    assert r["traffic"] is None or r["traffic"] > 0
    for m in r["memory"]:
        assert m["bound"] == "hbm" and m["peak"] == 8000.0 and 0 < m["frac"] < 1
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1 and "sample" in c
    assert d["value"] > 20 * c["value"]          # a GPU path that routed through the CPU oracle could not be this far ahead


def test_plain_bench_times_only_the_steps_and_dumps_the_same_outputs_every_run(tmp_path):
    import numpy as np
    runs = []
    for k in range(2):
        d = _bench("--gpus", "1", "--steps", "40", "--warmup", "5", "--replay", "20000", "--dump-outputs", str(tmp_path / str(k)))
        assert d["steps"] == 40 and d["warmup"] == 5 and "grad-steps" in d["metric"] and d["unit"] == "grad-steps/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f32"
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 0.01
        assert d["roofline"] is None and d["cpu_baseline"] is None       # --full only
        assert not {"repeats", "learn_loop", "success_rate"} & set(d)
        runs.append(d)
    names = sorted(os.listdir(tmp_path / "0"))
    assert names == sorted(os.listdir(tmp_path / "1")) and all(n.endswith(".npy") for n in names)
    assert any(n.startswith("param_") for n in names) and "metric_policy_loss.npy" in names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "0" / n), np.load(tmp_path / "1" / n)
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and a.shape == b.shape, n
        assert np.array_equal(a, b), n
        assert np.all(np.isfinite(a)), n
        total += a.nbytes
    assert total <= 64 << 20
    pl = float(np.load(tmp_path / "0" / "metric_policy_loss.npy"))      # the line's losses are the dumped step's
    assert abs(pl - runs[0]["losses"]["policy_loss"]) <= 1e-6 * max(1.0, abs(pl))


def test_bench_refuses_a_substituted_library():
    e = dict(os.environ, GRL_LIBRARY="/nonexistent/libgrl.so")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"], cwd=ROOT, env=e,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "GRL_LIBRARY" in (out.stderr + out.stdout)
