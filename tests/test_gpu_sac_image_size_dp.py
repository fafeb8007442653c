"""Data parallelism at an image size other than 64x64: two processes on the box's one MI355X, 50x50 depth images, 8 rows per
rank -- the light exchange case of tests/test_gpu_data_parallel.py (two-shot over two explicit minibatches): gradient buckets
and staged-split shapes come from the handle's layout, the result is bit-identical to the rank-ordered float32 sum."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import parity_util as pu
import sac_image_size_util as su
from grasp_rl import _capi

pytestmark = pytest.mark.gpu
os.environ.setdefault("OMP_NUM_THREADS", "4")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "4")
HW, ROWS, STEPS = 50, 8, 2


def _rank_ordered_reference(case, lo, hi, world):
    ref = pu.engine_setup(case)
    for s in range(STEPS):
        ref.compute_grads(case["idx"][s:s + 1, lo:hi], case["eps"][s:s + 1, lo:hi])
        g = torch.from_numpy(ref.fetch("grads", (ref.n_trainable,)))
        parts = [torch.empty_like(g) for _ in range(world)]
        dist.all_gather(parts, g)
        total = parts[0].numpy().copy()
        for p in parts[1:]:
            total += p.numpy()
        ref.store("grads", total)
        ref.apply_grads(1.0 / world)
    ref.synchronize()
    P = ref.get_parameters()
    ref.close()
    return P


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["GRL_TUNE"] = "dp_timeout_ms=20000"
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "gloo_store"), rank=rank, world_size=world)
    from grasp_rl.parallel import DataParallelInGraph
    case = su.make_case(HW, B=ROWS * world, n_replay=32, n_steps=STEPS)
    cfg = _capi.GrlConfig.from_buffer_copy(case["cfg"])
    cfg.batch_size = ROWS
    case["cfg"] = cfg
    lo, hi = rank * ROWS, (rank + 1) * ROWS
    Pref = _rank_ordered_reference(case, lo, hi, world)
    for overlap in (False, True):            # (overlap: the staged split -- its dense shapes are the handle's, K = 64 * 2 * 2 here)
        eng = pu.engine_setup(case)
        dp = DataParallelInGraph(eng, overlap=overlap, mode="twoshot")
        dp.train(STEPS, case["idx"][:, lo:hi], case["eps"][:, lo:hi])
        assert dp.check() == STEPS
        P = eng.get_parameters()
        for k in P:
            assert np.array_equal(P[k], Pref[k]), "overlap %s: differs from the rank-ordered sum: %s" % (overlap, k)
        dp.close()
        eng.close()
    np.savez(os.path.join(out_dir, "dp_%d.npz" % rank), **{k.replace("/", "|"): v for k, v in P.items()})
    dist.destroy_process_group()


def test_two_ranks_on_one_device_at_50(tmp_path, monkeypatch):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    monkeypatch.setenv("OPENBLAS_NUM_THREADS", "4")
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = (np.load(os.path.join(str(tmp_path), "dp_%d.npz" % r)) for r in range(2))
    assert a["model|pi|cnn_fc1|w:0"].shape == (su.dense_k(HW), 512)
    for k in a.files:
        assert np.array_equal(a[k], b[k]), "replicas diverged: " + k
