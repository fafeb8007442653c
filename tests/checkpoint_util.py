"""Shared by tests/test_hostemu_checkpoint.py (emulation build, CPU) and tests/test_gpu_checkpoint.py (MI355X): the
checkpoint -> destroy -> restore -> continue procedure and its comparisons.  Every comparison is exact: arenas are compared
as raw 32-bit words (NaN patterns included), metrics as the floats the library reports."""
import ctypes

import numpy as np

import parity_util as pu
import q_parity_util as qu
from grasp_rl import _capi
from grasp_rl.engine import QEngine, SacEngine


def words(eng, arena):
    """An arena of the engine as host uint32 words."""
    return np.ascontiguousarray(eng.be.to_host(arena)).view(np.uint32)


def saved_mask(eng):
    """Boolean mask over the WORDS of the replay arena: True where a checkpoint of this engine stores the word."""
    size = eng.replay_size()
    mask = np.zeros(int(eng.replay.shape[0]), bool)
    for seg in eng.replay_segments():
        lo, hi = eng._segment_span(seg, size)
        assert not mask[lo:hi].any(), "replay segments overlap"
        mask[lo:hi] = True
    return mask


def assert_same_training_state(a, b, what=""):
    sa, sb = words(a, a.state), words(b, b.state)
    assert np.array_equal(sa, sb), "%s: state arenas differ in %d words" % (what, int((sa != sb).sum()))
    assert a.replay_size() == b.replay_size(), what
    ma, mb = saved_mask(a), saved_mask(b)
    assert np.array_equal(ma, mb), what
    ra, rb = words(a, a.replay), words(b, b.replay)
    assert np.array_equal(ra[ma], rb[mb]), "%s: saved replay segments differ in %d words" % (what, int((ra[ma] != rb[mb]).sum()))
    assert a.export_state() == b.export_state(), "%s: handle state differs" % what
    ka, kb = a.metrics(), b.metrics()
    for k in ka:
        assert np.float32(ka[k]).tobytes() == np.float32(kb[k]).tobytes(), "%s: metric %s %r != %r" % (what, k, ka[k], kb[k])


def fill_past_one_wrap(eng, tr, extra=None):
    """The whole ring once, then `extra` (default: half) of it again: rp_pos < rp_size == capacity."""
    n = int(eng.cfg.replay_capacity)
    assert tr["rew"].shape[0] == n
    eng.replay_add(tr["obs"], tr["act"], tr["rew"], tr["next_obs"], tr["done"])
    k = n // 2 if extra is None else extra
    # (the second pass stores the rows in reverse order: the ring's head differs from what the first pass left there)
    sel = np.arange(n)[::-1][:k]
    eng.replay_add(tr["obs"][sel], tr["act"][sel], tr["rew"][sel], tr["next_obs"][sel], tr["done"][sel])
    assert eng.replay_size() == n


class SacRun:
    """One SAC engine of a parity_util case; `factory()` builds another on the same configuration."""

    def __init__(self, backend_factory, lib_path=None, **case_kw):
        self.case = pu.make_case(**case_kw)
        self.backend_factory, self.lib_path = backend_factory, lib_path

    def bare(self, cfg=None):
        return SacEngine(self.case["cfg"] if cfg is None else cfg, backend=self.backend_factory(), lib_path=self.lib_path)

    def prepared(self, wrap=True):
        eng = self.bare()
        eng.set_parameters(self.case["params"])
        st = self.case["stats"]
        eng.set_obs_stats(st["mean"], st["var"], st["ret_var"])
        tr = self.case["tr"]
        if wrap:
            fill_past_one_wrap(eng, tr)
        else:
            k = tr["rew"].shape[0] * 2 // 3
            eng.replay_add(tr["obs"][:k], tr["act"][:k], tr["rew"][:k], tr["next_obs"][:k], tr["done"][:k])
        return eng

    def train(self, eng, n):
        eng.train(n)


class QRun:
    def __init__(self, backend_factory, lib_path=None, name="bdq", prioritized=False, n_replay=40, **over):
        kw = dict(qu.CASES[name])
        kw.update(over)
        kw.pop("route", None)
        self.case = qu.make_q_case(n_replay=n_replay, **kw)
        self.prioritized = prioritized
        if prioritized:
            c = self.case["cfg"]
            c.q_per, c.q_per_alpha, c.q_per_eps, c.q_per_alpha64 = 1, 0.6, 1e-6, 0.6
        self.backend_factory, self.lib_path = backend_factory, lib_path

    def bare(self, cfg=None):
        return QEngine(self.case["cfg"] if cfg is None else cfg, backend=self.backend_factory(), lib_path=self.lib_path)

    def prepared(self, wrap=True):
        eng = self.bare()
        eng.set_parameters(self.case["params"])
        st = self.case["stats"]
        eng.set_obs_stats(st["mean"], st["var"], st["ret_var"])
        tr = self.case["tr"]
        if wrap:
            fill_past_one_wrap(eng, tr)
        else:
            k = tr["rew"].shape[0] * 2 // 3
            eng.replay_add(tr["obs"][:k], tr["act"][:k], tr["rew"][:k], tr["next_obs"][:k], tr["done"][:k])
        return eng

    def train(self, eng, n):
        if self.prioritized:
            eng.train_per(n, beta=0.4)
        else:
            eng.train(n)


def continuation(run, path, n, before=None, after=None, wrap=True, include_replay=True, poison=False):
    """Run A: prepare, n updates, [before], [after], n more.  Run B: prepare, n updates, [before], save_state, destroy, a new
    engine of the same configuration, load_state, [poison what the checkpoint does not cover], [after], n more.  Returns
    (A, B) for the caller to compare and close."""
    a, b = run.prepared(wrap), run.prepared(wrap)
    for e in (a, b):
        run.train(e, n)
        if before is not None:
            before(e)
    if wrap:
        hdr = _capi.GrlStateHeader.from_buffer_copy(a.export_state()[:ctypes.sizeof(_capi.GrlStateHeader)])
        assert 0 < hdr.replay_pos < hdr.replay_size == a.cfg.replay_capacity
    meta = b.save_state(path, include_replay=include_replay)
    b.close()
    b = run.bare()
    b.load_state(path)
    if poison:
        keep = saved_mask(b)
        r = words(b, b.replay).copy()
        r[~keep] = 0xFFFFFFFF
        b.be.write(b.replay, r.view(np.float32))
        b.be.synchronize()
    for e in (a, b):
        if after is not None:
            after(e)
        run.train(e, n)
    return a, b, meta
