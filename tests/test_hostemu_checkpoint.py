"""Checkpoint and resume of the full training state at the engine layer, on CPU through the TEST-ONLY emulation build
(tests/test_hostemu_plan.py): a run that is checkpointed, destroyed, restored into a new engine and continued must be
bit-identical to the run that was never interrupted.  No tolerances: arenas are compared as raw words."""
import os
import shutil

import numpy as np
import pytest

import checkpoint_util as cu
from grasp_rl import _capi
from grasp_rl._capi import GrlError
from hostemu_backend import NumpyHostBackend

N = 3       # updates before and after the checkpoint


def _sac(lib, **kw):
    return cu.SacRun(NumpyHostBackend, lib, **kw)


def _q(lib, **kw):
    return cu.QRun(NumpyHostBackend, lib, **kw)


RUNS = {
    "sac_mlp": lambda lib: _sac(lib, extractor="mlp", B=16, n_replay=64),
    "sac_depth_cnn": lambda lib: _sac(lib, extractor="augmented", kind="depth", B=4, n_replay=16),
    "sac_rgbd_u8": lambda lib: _sac(lib, extractor="augmented", kind="rgbd", B=3, n_replay=12, rgb_u8=True),
    "dqn_uniform": lambda lib: _q(lib, name="dqn"),
    "bdq_per": lambda lib: _q(lib, name="bdq", prioritized=True, n_replay=2100),      # three blocks of the priority tree
}


@pytest.mark.parametrize("name", list(RUNS))
def test_engine_continuation_is_bit_identical(hostemu_lib, tmp_path, name):
    run = RUNS[name](hostemu_lib)
    a, b, meta = cu.continuation(run, str(tmp_path / "ck"), N)
    cu.assert_same_training_state(a, b, name)
    assert meta["replay_size"] == a.cfg.replay_capacity and 0 < meta["replay_pos"] < meta["replay_size"]
    assert sorted(os.listdir(tmp_path)) == ["ck"]           # no .tmp / .old left behind
    a.close(); b.close()


def _obs_rows(run, k0, n):
    return np.ascontiguousarray(run.case["tr"]["obs"][k0:k0 + n], np.float32)


@pytest.mark.parametrize("kind", ["mlp", "depth"])
def test_checkpoint_between_two_observe_calls(hostemu_lib, tmp_path, kind):
    """grl_observe | checkpoint | grl_observe -> grl_replay_add_observed: the `previous` rows live in the work arena and
    travel in the handle blob; the statistics were updated ONCE before the checkpoint (odd: the double-buffered count)."""
    run = (_sac(hostemu_lib, extractor="mlp", B=16, n_replay=64) if kind == "mlp"
           else _sac(hostemu_lib, extractor="augmented", kind="depth", B=4, n_replay=16))
    n, A = 4, run.case["cfg"].act_dim
    rng = np.random.default_rng(5)
    act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
    rew, done = rng.normal(size=n).astype(np.float32), np.array([0, 1, 0, 0], np.float32)

    def before(e):
        e.observe(_obs_rows(run, 0, n), update_stats=True)

    def after(e):
        e.observe(_obs_rows(run, 4, n), update_stats=True)
        e.replay_add_observed(act, rew, done, [1], _obs_rows(run, 9, 1))
        out = e.act(n, deterministic=True, raw=True, observed=True)
        after.acts.append(out)

    after.acts = []
    a, b, _ = cu.continuation(run, str(tmp_path / "ck"), N, before=before, after=after)
    cu.assert_same_training_state(a, b, kind)
    assert np.array_equal(after.acts[0].view(np.uint32), after.acts[1].view(np.uint32))
    a.close(); b.close()


@pytest.mark.parametrize("updates", [1, 3, 2])
def test_running_statistics_double_buffer(hostemu_lib, tmp_path, updates):
    """grl_norm_update an odd (and an even) number of times before the checkpoint, once more after it."""
    run = _sac(hostemu_lib, extractor="mlp", B=16, n_replay=64)

    def before(e):
        for k in range(updates):
            e.norm_update(_obs_rows(run, 4 * k, 4))

    def after(e):
        e.norm_update(_obs_rows(run, 20, 4))

    a, b, _ = cu.continuation(run, str(tmp_path / "ck"), N, before=before, after=after)
    cu.assert_same_training_state(a, b)
    shape = (run.case["cfg"].obs_dim,)
    for x, y in zip(a.get_obs_stats(shape), b.get_obs_stats(shape)):
        assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))
    a.close(); b.close()


@pytest.mark.parametrize("name", ["sac_mlp", "bdq_per"])
def test_checkpoint_without_the_ring(hostemu_lib, tmp_path, name):
    run = RUNS[name](hostemu_lib)
    src = run.prepared()
    run.train(src, N)
    src.save_state(str(tmp_path / "ck"), include_replay=False)
    assert not [f for f in os.listdir(tmp_path / "ck") if f.startswith("replay_")]
    dst = run.bare()
    dst.load_state(str(tmp_path / "ck"))
    sa, sb = cu.words(src, src.state), cu.words(dst, dst.state)
    # parameters, optimiser state, statistics and counters: the state arena, but for the device mirror of the ring size
    diff = np.flatnonzero(sa != sb)
    assert len(diff) == 1 and int(sa[diff[0]]) == src.replay_size() and int(sb[diff[0]]) == 0, diff
    for (k, p), q in zip(src.get_parameters().items(), dst.get_parameters().values()):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), k
    assert dst.replay_size() == 0
    fresh = run.bare()
    for e in (dst, fresh):
        with pytest.raises(GrlError, match="replay buffer is empty"):
            run.train(e, 1)
    # ... and it refills like a new ring
    tr = run.case["tr"]
    for e in (dst,):
        e.replay_add(tr["obs"], tr["act"], tr["rew"], tr["next_obs"], tr["done"])
        run.train(e, 2)
        assert all(np.isfinite(v) for v in e.metrics().values())
    src.close(); dst.close(); fresh.close()


def _snapshot(e):
    return cu.words(e, e.state).copy(), cu.words(e, e.replay).copy(), cu.words(e, e.work).copy(), e.export_state()


def _assert_unchanged_and_usable(run, e, snap):
    now = _snapshot(e)
    for x, y in zip(snap[:3], now[:3]):
        assert np.array_equal(x, y)
    assert snap[3] == now[3]
    run.train(e, 1)


@pytest.mark.parametrize("field,value,names", [("batch_size", 8, "batch_size"), ("layers", 32, "layers"),
                                               ("replay_capacity", 48, "replay_capacity")])
def test_checkpoint_of_another_configuration_is_refused(hostemu_lib, tmp_path, field, value, names):
    run = RUNS["sac_mlp"](hostemu_lib)
    src = run.prepared()
    run.train(src, N)
    src.save_state(str(tmp_path / "ck"))
    other = _sac(hostemu_lib, extractor="mlp", B=16, n_replay=64)
    if field == "layers":
        other.case["cfg"].layers[1] = value
    else:
        setattr(other.case["cfg"], field, value)
    dst = other.bare()
    tr = run.case["tr"]
    dst.replay_add(tr["obs"][:40], tr["act"][:40], tr["rew"][:40], tr["next_obs"][:40], tr["done"][:40])
    snap = _snapshot(dst)
    with pytest.raises(GrlError, match="grl_config." + names):
        dst.load_state(str(tmp_path / "ck"))
    _assert_unchanged_and_usable(other, dst, snap)
    src.close(); dst.close()


@pytest.mark.parametrize("damage", ["truncated", "magic", "short_state", "missing_segment", "version"])
def test_damaged_checkpoint_is_refused(hostemu_lib, tmp_path, damage):
    run = RUNS["bdq_per"](hostemu_lib)
    src = run.prepared()
    run.train(src, N)
    ck = str(tmp_path / "ck")
    src.save_state(ck)
    hb = os.path.join(ck, "handle.bin")
    blob = open(hb, "rb").read()
    if damage == "truncated":
        open(hb, "wb").write(blob[:len(blob) - 5])
    elif damage == "magic":
        open(hb, "wb").write(b"XXXX" + blob[4:])
    elif damage == "short_state":
        sb = os.path.join(ck, "state.bin")
        open(sb, "wb").write(open(sb, "rb").read()[:-4])
    elif damage == "missing_segment":
        os.remove(os.path.join(ck, "replay_%d.bin" % (len(src.replay_segments()) - 1)))
    else:
        import json
        meta = json.load(open(os.path.join(ck, "meta.json")))
        meta["grl_version"] += 1
        json.dump(meta, open(os.path.join(ck, "meta.json"), "w"))
    dst = run.prepared(wrap=False)
    snap = _snapshot(dst)
    with pytest.raises(GrlError):
        dst.load_state(ck)
    _assert_unchanged_and_usable(run, dst, snap)
    src.close(); dst.close()


def test_import_rejects_short_and_foreign_blobs_by_name(hostemu_lib):
    run = RUNS["sac_mlp"](hostemu_lib)
    e = run.prepared()
    blob = e.export_state()
    for bad, msg in ((blob[:10], "truncated"), (blob[:-1], "truncated"), (b"\0" * len(blob), "magic"), (blob + b"\0", "truncated")):
        with pytest.raises(GrlError, match=msg):
            e.import_state(bad)
    e.import_state(blob)
    assert e.export_state() == blob
    segs = (_capi.GrlSegment * 2)()
    assert e.lib.grl_replay_segments(e.h, 2, segs) < 0          # cap too small
    e.close()


class _FailingBackend(NumpyHostBackend):
    """to_host raises at its `fail_at`-th call (save_state: state arena, then one call per replay segment)."""

    def __init__(self, fail_at):
        self.calls, self.fail_at = 0, fail_at

    def to_host(self, a):
        self.calls += 1
        if self.calls == self.fail_at:
            raise RuntimeError("killed")
        return super().to_host(a)


def test_interrupted_save_keeps_the_previous_checkpoint(hostemu_lib, tmp_path):
    run = cu.QRun(lambda: _FailingBackend(fail_at=0), hostemu_lib, name="bdq", prioritized=True, n_replay=2100)
    ck = str(tmp_path / "ck")
    e = run.prepared()
    run.train(e, N)
    e.save_state(ck)
    first = _snapshot(e)
    run.train(e, N)
    e.be.calls, e.be.fail_at = 0, 3        # state arena, first segment, then dies in the second
    with pytest.raises(RuntimeError, match="killed"):
        e.save_state(ck)
    assert os.path.isdir(ck + ".tmp") and os.path.exists(os.path.join(ck + ".tmp", "replay_0.bin"))
    back = run.bare()
    back.load_state(ck)
    now = _snapshot(back)
    assert np.array_equal(first[0], now[0]) and first[3] == now[3]
    keep = cu.saved_mask(back)
    assert np.array_equal(first[1][keep], now[1][keep])
    # a later save cleans the debris up and replaces the checkpoint
    e.be.fail_at = 0
    e.save_state(ck)
    assert sorted(os.listdir(tmp_path)) == ["ck"]
    # a save that died between its two renames left `<dir>.old` only: it still loads
    os.rename(ck, ck + ".old")
    again = run.bare()
    again.load_state(ck)
    assert np.array_equal(cu.words(again, again.state), cu.words(e, e.state))
    shutil.rmtree(ck + ".old")
    e.close(); back.close(); again.close()


@pytest.mark.parametrize("name", ["sac_depth_cnn", "sac_rgbd_u8", "bdq_per", "dqn_uniform"])
def test_segments_cover_what_training_reads(hostemu_lib, tmp_path, name):
    """A partly filled ring: after load_state every word of the replay arena that the checkpoint does NOT store is
    overwritten with 0xFFFFFFFF (a NaN); more transitions arrive, training continues -- still bit-identical."""
    run = RUNS[name](hostemu_lib)
    tr = run.case["tr"]
    k = tr["rew"].shape[0] * 2 // 3

    def after(e):
        e.replay_add(tr["obs"][k:k + 3], tr["act"][k:k + 3], tr["rew"][k:k + 3], tr["next_obs"][k:k + 3], tr["done"][k:k + 3])

    a, b, meta = cu.continuation(run, str(tmp_path / "ck"), N, after=after, wrap=False, poison=True)
    assert meta["replay_size"] == k
    cu.assert_same_training_state(a, b, name)
    segs = a.replay_segments()
    spans = sorted((off, off + (rb * rows if rows else rb)) for off, rb, rows in segs)
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:])) and spans[-1][1] <= a.sizes.replay_bytes
    assert os.path.getsize(os.path.join(str(tmp_path / "ck"), "replay_0.bin")) == segs[0][1] * k      # filled rows only
    a.close(); b.close()
