"""Wide DQN / BDQ handles on the MI355X through the C ABI (tests/q_wide_util.py): q_sumsq_kernel / q_clip_adam_kernel
(csrc/q_wide_kernels.h) over the tile table and the layer-0 partial sums added by the matrix-core chains, against the float64
reference with the wide yardstick; the route asserted from the plan dump on both sides of 131 072 floats; act rows, multi-update
calls, run-to-run bits, checkpoint and two replicas on one device."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import q_wide_util as qw
from grasp_rl import _capi

pytestmark = pytest.mark.gpu
os.environ.setdefault("OMP_NUM_THREADS", "4")          # (inherited by the spawned replicas: tests/test_gpu_data_parallel.py)
os.environ.setdefault("OPENBLAS_NUM_THREADS", "4")


def test_131072_floats_is_not_wide_and_keeps_the_parent_plan(monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    plan = qw.edge_plan(2048, lambda: capfd.readouterr().err)
    assert "q_wide" not in plan and "in one launch: no" in plan, plan
    l0 = [ln for ln in plan.splitlines() if ln.startswith("grl plan: q_l0")]
    assert l0 and all(ln.endswith("probs 6  tiles 6") for ln in l0), plan          # layer 0 uncut: one tile per problem


def test_131136_floats_is_the_first_wide_handle(monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    plan = qw.edge_plan(2049, lambda: capfd.readouterr().err)
    line = qw.wide_line(plan)
    assert line is not None and "q_sumsq + q_clip_adam" in line, plan
    assert "%d tiles" % (2 * ((2049 * 64 + qw.TILE - 1) // qw.TILE) + 2 + 2 + 6) in line, line
    split = int(line.split("q_l0: ")[1].split()[0])
    assert 6 * split >= 64 and 6 * (split - 1) < 64, line
    assert "matrix-core stages" in plan and "grl plan: q_l0" in plan


@pytest.mark.parametrize("name", qw.PARITY_CASES)
def test_update_matches_the_float64_reference(name, monkeypatch, capfd):
    """forward, every gradient tensor, three updates with the target copy, the clipped gradient in the bucket: the engine within
    the existing tolerance + 4 d_ref of float64 (figures printed per quantity)"""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    qw.run_and_compare_wide(name)
    out = capfd.readouterr()
    print(out.out)
    line = qw.wide_line(out.err)
    assert line is not None, out.err
    assert ("q_l0: 1 partial" in line) == bool(qw.WIDE_CASES[name].get("layer_norm")), line


@pytest.mark.parametrize("n", qw.ACT_NS)
@pytest.mark.parametrize("name", ["dqn8192_B32", "bdq8192_B16"])
def test_act_bins_equal_the_argmax_of_the_reference(name, n):
    qw.act_check(name, n)


@pytest.mark.parametrize("name", ["dqn8192_B32", "bdq8192_B16", "dqn8192_per", "dqn8192_ln"])
def test_one_call_of_n_updates_equals_n_calls_and_a_second_run(name):
    qw.multi_update_check(name, lambda: None)


def test_checkpoint_and_continue_on_a_new_handle(tmp_path):
    qw.checkpoint_check("dqn8192_B32", lambda: None, str(tmp_path / "ck"))


# ---------------------------------------------------------------------------------------------------------------------
# two replicas on the one device (the pattern of tests/test_gpu_data_parallel.py: _q_ingraph_worker)
STEPS = 3


def _init_gloo(rank, world, out_dir):
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "gloo_store"), rank=rank, world_size=world)


def _wide_dp_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["GRL_TUNE"] = "dp_timeout_ms=20000"
    _init_gloo(rank, world, out_dir)
    import q_layer_norm_util as ql
    from grasp_rl.parallel import DataParallelInGraph
    case = dict(qw.make_wide_case("dqn8192_B32"))             # pixel inputs: the clip is active on the wide variables
    Bq = case["B"]
    cfg = _capi.GrlConfig.from_buffer_copy(case["cfg"])
    cfg.batch_size = Bq // world
    case["cfg"] = cfg
    lo, hi = rank * (Bq // world), (rank + 1) * (Bq // world)
    # reference: every rank's bucket added in rank order on the host, applied with grad_scale 1 / W on a plain handle
    ref = ql.engine_setup(case)
    clip = float(cfg.q_grad_clip)
    for s in range(STEPS):
        ref.compute_grads(case["idx"][s:s + 1, lo:hi], case["weights"][s:s + 1, lo:hi])
        g = torch.from_numpy(ref.fetch("grads", (ref.n_trainable,)))
        parts = [torch.empty_like(g) for _ in range(world)]
        dist.all_gather(parts, g)
        total = parts[0].numpy().copy()
        for p in parts[1:]:
            total += p.numpy()
        ref.store("grads", total)
        sums = ref.get_gradients()
        ref.apply_grads(1.0 / world)
        if s == 0:        # the clip is applied to the MEAN: the bucket holds the sum clipped at W c
            after = ref.get_gradients()
            wide = [n for n, v in sums.items() if v.size > qw.WIDE_MIN]
            assert len(wide) == 2
            for n in wide:
                norm = lambda a: float(np.sqrt((np.asarray(a, np.float64) ** 2).sum()))
                assert norm(sums[n]) / world > clip                              # active on the mean
                assert abs(norm(after[n]) / world - clip) <= qw.clip_rel(sums[n].size) * clip, (n, norm(after[n]))
    ref.synchronize()
    Pref = ref.get_parameters()
    ref.close()
    eng = ql.engine_setup(case)
    dp = DataParallelInGraph(eng, mode="auto")
    dp.train(STEPS, case["idx"][:, lo:hi], case["weights"][:, lo:hi])
    assert dp.check() == STEPS
    P = eng.get_parameters()
    for k in P:
        assert np.array_equal(P[k], Pref[k]), "differs from the rank-ordered sum: %s" % k
    dp.train(2)                                               # device RNG: same seed and replay contents on every rank
    assert dp.check() == STEPS + 2
    np.savez(os.path.join(out_dir, "wide_%d.npz" % rank), **{k.replace("/", "|"): v for k, v in eng.get_parameters().items()})
    dp.close()
    eng.close()
    dist.destroy_process_group()


def test_two_replicas_on_one_device_clip_the_mean_and_stay_identical(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_wide_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "wide_%d.npz" % r)) for r in range(2)]
    for k in parts[0].files:
        assert np.array_equal(parts[0][k], parts[1][k]), "replicas diverged: %s" % k
