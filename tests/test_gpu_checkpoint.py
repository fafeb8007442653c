"""Checkpoint and resume on the MI355X (real library, TorchCudaBackend with the page-locked staging of save_state /
load_state): checkpoint -> destroy -> new engine -> restore -> continue is bit-identical to the uninterrupted run.  The
procedure and the exact comparisons are those of tests/test_hostemu_checkpoint.py (tests/checkpoint_util.py)."""
import os

import numpy as np
import pytest

import checkpoint_util as cu
from grasp_rl._capi import GrlError
from grasp_rl.engine import TorchCudaBackend

pytestmark = pytest.mark.gpu


def _sac(**kw):
    return cu.SacRun(TorchCudaBackend, None, **kw)


def test_sac_depth_b256_inside_graphed_multi_update_calls(tmp_path, capfd, monkeypatch):
    """2 x 40 updates per call with the default graph_updates: the `gather_ride` plan, replayed as hipGraphs."""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    run = _sac(extractor="augmented", kind="depth", B=256, n_replay=600)
    a, b, meta = cu.continuation(run, str(tmp_path / "ck"), 40)
    assert "gather_ride" in capfd.readouterr().err
    cu.assert_same_training_state(a, b, "sac_depth")
    assert meta["replay_size"] == 600
    a.close(); b.close()


def test_sac_rgbd_with_byte_colours(tmp_path):
    run = _sac(extractor="augmented", kind="rgbd", B=64, n_replay=200, rgb_u8=True)
    a, b, _ = cu.continuation(run, str(tmp_path / "ck"), 12)
    cu.assert_same_training_state(a, b, "sac_rgbd")
    a.close(); b.close()


def test_sac_depth_between_two_observe_calls_with_odd_statistics_updates(tmp_path):
    run = _sac(extractor="augmented", kind="depth", B=32, n_replay=96)
    n, A = 4, run.case["cfg"].act_dim
    rng = np.random.default_rng(5)
    act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
    rew, done = rng.normal(size=n).astype(np.float32), np.array([0, 1, 0, 0], np.float32)
    obs = run.case["tr"]["obs"]
    acts = []

    def before(e):
        e.observe(np.ascontiguousarray(obs[0:4]), update_stats=True)

    def after(e):
        e.observe(np.ascontiguousarray(obs[4:8]), update_stats=True)
        e.replay_add_observed(act, rew, done, [1], np.ascontiguousarray(obs[9:10]))
        acts.append(e.act(n, deterministic=True, raw=True, observed=True))

    a, b, _ = cu.continuation(run, str(tmp_path / "ck"), 5, before=before, after=after)
    cu.assert_same_training_state(a, b, "observe")
    assert np.array_equal(acts[0].view(np.uint32), acts[1].view(np.uint32))
    a.close(); b.close()


@pytest.mark.parametrize("wrap", [True, False])
def test_bdq_prioritised(tmp_path, wrap):
    """wrap=False: a partly filled ring, and every word the checkpoint does not store poisoned after the load."""
    run = cu.QRun(TorchCudaBackend, None, name="bdq_baseline_config3", prioritized=True, n_replay=2100)
    a, b, _ = cu.continuation(run, str(tmp_path / "ck"), 20, wrap=wrap, poison=not wrap)
    cu.assert_same_training_state(a, b, "bdq_per")
    a.close(); b.close()


def test_without_the_ring_and_refusals(tmp_path):
    run = _sac(extractor="augmented", kind="depth", B=32, n_replay=96)
    src = run.prepared()
    run.train(src, 4)
    ck = str(tmp_path / "ck")
    src.save_state(ck, include_replay=False)
    dst = run.bare()
    dst.load_state(ck)
    assert dst.replay_size() == 0
    for (k, p), q in zip(src.get_parameters().items(), dst.get_parameters().values()):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), k
    with pytest.raises(GrlError, match="replay buffer is empty"):
        dst.train(1)
    other = _sac(extractor="augmented", kind="depth", B=16, n_replay=96)
    eng = other.prepared()
    before = cu.words(eng, eng.state).copy()
    with pytest.raises(GrlError, match="grl_config.batch_size"):
        eng.load_state(ck)
    assert np.array_equal(before, cu.words(eng, eng.state))
    eng.train(2)
    assert os.path.isdir(ck)
    src.close(); dst.close(); eng.close()
