"""bench.py's host-side helpers, without a GPU: `--dump-outputs` writes float32 / float64 .npy files under a size cap (a fixed
sample past it), and the untimed warm-up call replays the graph shapes of the timed call."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_helpers_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_float_arrays(tmp_path):
    bench = _bench()
    arrays = {"param/model/pi/fc0/kernel:0": np.arange(12, dtype=np.float32).reshape(3, 4), "metric/policy_loss": 1.5,
              "sampled_indices": np.array([3, 1 << 40], np.int64), "half": np.ones(3, np.float16)}
    names = bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert names == sorted(os.listdir(tmp_path / "out"))
    assert names == ["half.npy", "metric_policy_loss.npy", "param_model_pi_fc0_kernel_0.npy", "sampled_indices.npy"]
    k = np.load(tmp_path / "out" / "param_model_pi_fc0_kernel_0.npy")
    assert k.dtype == np.float32 and np.array_equal(k, arrays["param/model/pi/fc0/kernel:0"])
    m = np.load(tmp_path / "out" / "metric_policy_loss.npy")
    assert m.dtype == np.float64 and float(m) == 1.5
    i = np.load(tmp_path / "out" / "sampled_indices.npy")
    assert i.dtype == np.float64 and i.tolist() == [3.0, float(1 << 40)]
    assert np.load(tmp_path / "out" / "half.npy").dtype == np.float32


def test_dump_outputs_samples_past_the_cap_the_same_way_every_time(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 80_000)
    rng = np.random.default_rng(1)
    arrays = {"big": rng.normal(size=40_000).astype(np.float32), "small": np.arange(100, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(a, b) and a.nbytes + 400 <= 80_000
    assert np.all(np.isin(a, arrays["big"]))                              # a sample of the elements, in their order
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"])


def test_warm_shape_keeps_the_graph_groups_of_the_timed_call():
    bench = _bench()
    for n in range(1, bench.WARM_MAX + 1):
        assert bench.warm_shape(n) == n
    for n in list(range(bench.WARM_MAX + 1, bench.WARM_MAX + 1000)) + [100_000, 123_457]:
        w = bench.warm_shape(n)
        assert bench.WARM_MAX - 64 < w <= bench.WARM_MAX and (n - w) % 64 == 0, n
