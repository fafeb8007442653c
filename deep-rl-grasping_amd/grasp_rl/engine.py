"""SacEngine -- thin Python owner of the device arenas + handle of libgrl.so.

The arithmetic of the SAC update (replay gather/normalise, CNN + MLP forward/backward, losses, Adam,
Polyak) runs in the HIP kernels behind the C ABI of include/grl.h; PyTorch-ROCm only provides the
device memory (four flat tensors), the stream and -- for data parallelism -- the RCCL all-reduce of
the flat gradient tensor.  There is no CPU fallback: constructing an engine without a HIP device or
without the built library raises.

Reference call sites this object stands behind: sb.SAC(...) construction and .learn()'s per-step
update at /root/reference/manipulation_main/training/sb_helper.py:104-128,175-177.
"""
import ctypes as C
import json
import os
import shutil
from collections import OrderedDict

import numpy as np

from . import _capi
from ._capi import GrlError, check


CHECKPOINT_FORMAT = 1
STAGE_BYTES = 256 << 20         # page-locked staging of save_state / load_state: two halves used in turn, never more than this


def _flush(f):
    f.flush()
    os.fsync(f.fileno())


def _sync_dir(path):
    """The directory entries themselves on the disk (a rename is durable only then)."""
    try:
        fd = os.open(path, os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass
    finally:
        os.close(fd)


def _release_staging(be):
    if hasattr(be, "release_staging"):
        be.release_staging()


def _read_chunks(be, t, lo, hi):
    """float32 elements [lo, hi) of arena `t` as successive host arrays (each valid until the next one is asked for)."""
    fn = getattr(be, "read_chunks", None)
    if fn is not None:
        yield from fn(t, lo, hi)
        return
    step = STAGE_BYTES // 8
    for a in range(lo, hi, step):
        yield be.to_host(t[a:min(hi, a + step)])


def _write_chunks(be, t, lo, hi, fill):
    """fill(array) loads the next float32 elements of [lo, hi) into a host array, which then goes to arena `t`."""
    fn = getattr(be, "write_chunks", None)
    if fn is not None:
        fn(t, lo, hi, fill)
        return
    step = STAGE_BYTES // 8
    for a in range(lo, hi, step):
        b = min(hi, a + step)
        buf = np.empty(b - a, np.float32)
        fill(buf)
        be.write(t[a:b], buf)
    be.synchronize()


class TorchCudaBackend:
    """Device memory = PyTorch-ROCm tensors; work is enqueued on a dedicated HIP stream."""

    def __init__(self, device="cuda:0"):
        import torch
        if not torch.cuda.is_available():
            raise GrlError("no HIP device visible to PyTorch: the grasp_rl engine runs only on an AMD GPU "
                           "(MI355X / gfx950); there is no CPU fallback")
        self.torch = torch
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.Stream(device=self.device)

    def alloc_f32(self, nbytes):
        t = self.torch.zeros((nbytes + 3) // 4, dtype=self.torch.float32, device=self.device)
        self.torch.cuda.synchronize(self.device)
        return t

    def ptr(self, t):
        return t.data_ptr()

    def stream_ptr(self):
        return self.stream.cuda_stream

    def to_device(self, arr):
        # allocated and filled ON the engine stream: the caching allocator then only hands the block to someone
        # else after work queued on this stream (the kernels that read it) has been ordered before the reuse
        with self.torch.cuda.stream(self.stream):
            t = self.torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
        return t

    def to_host(self, t):
        self.stream.synchronize()
        return t.detach().cpu().numpy()

    def write(self, view, arr):
        with self.torch.cuda.stream(self.stream):
            view.copy_(self.torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).reshape(view.shape),
                       non_blocking=False)

    def synchronize(self):
        self.stream.synchronize()

    def stream_context(self):
        return self.torch.cuda.stream(self.stream)

    def comm_fork(self):
        """Marks the current end of the engine stream: a later `comm_context(fork)` starts its work there."""
        ev = self.torch.cuda.Event()
        ev.record(self.stream)
        return ev

    def comm_context(self, fork=None):
        """Context whose work runs on a second stream, ordered after `fork` (default: everything enqueued on the engine
        stream so far): the exchange of a finished gradient bucket, overlapping what the engine stream does next."""
        if getattr(self, "comm", None) is None:
            self.comm = self.torch.cuda.Stream(device=self.device)
        if fork is None:
            self.comm.wait_stream(self.stream)
        else:
            self.comm.wait_event(fork)
        return self.torch.cuda.stream(self.comm)

    def comm_join(self):
        """Engine stream waits for the second stream."""
        if getattr(self, "comm", None) is not None:
            self.stream.wait_stream(self.comm)

    def as_torch(self, t):
        return t

    # ---- checkpoint I/O: arena <-> host through ONE page-locked buffer of at most STAGE_BYTES, its two halves used in
    # turn, so that the device copy of chunk k + 1 runs while the caller writes (reads) chunk k to (from) the file
    def _staging(self, n):
        want = min(STAGE_BYTES // 4, 2 * max(int(n), 1))
        want += want & 1
        st = getattr(self, "_stage", None)
        if st is None or st.numel() < want:
            self._stage = st = self.torch.empty(want, dtype=self.torch.float32).pin_memory()
        half = st.numel() // 2
        return [st[:half], st[half:2 * half]], half

    def release_staging(self):
        """Frees the page-locked buffer (up to STAGE_BYTES): one save / load allocates it once and gives it back."""
        self.stream.synchronize()
        self._stage = None

    def staging_bytes(self):
        st = getattr(self, "_stage", None)
        return 0 if st is None else int(st.numel()) * 4

    def read_chunks(self, t, lo, hi):
        torch = self.torch
        if hi <= lo:
            return
        halves, half = self._staging(hi - lo)
        evs = [torch.cuda.Event(), torch.cuda.Event()]

        def issue(k, a):
            b = min(hi, a + half)
            with torch.cuda.stream(self.stream):
                halves[k][:b - a].copy_(t[a:b], non_blocking=True)
                evs[k].record(self.stream)
            return b - a

        a, k = lo, 0
        m = issue(k, a)
        while True:
            nxt = a + m
            m_next = issue(k ^ 1, nxt) if nxt < hi else 0
            evs[k].synchronize()
            yield halves[k][:m].numpy()
            if not m_next:
                break
            a, m, k = nxt, m_next, k ^ 1

    def write_chunks(self, t, lo, hi, fill):
        torch = self.torch
        if hi <= lo:
            return
        halves, half = self._staging(hi - lo)
        evs = [torch.cuda.Event(), torch.cuda.Event()]
        used = [False, False]
        a, k = lo, 0
        while a < hi:
            b = min(hi, a + half)
            if used[k]:
                evs[k].synchronize()
            fill(halves[k][:b - a].numpy())
            with torch.cuda.stream(self.stream):
                t[a:b].copy_(halves[k][:b - a], non_blocking=True)
                evs[k].record(self.stream)
            used[k] = True
            a, k = b, k ^ 1
        self.stream.synchronize()


class SacEngine:
    def __init__(self, cfg, backend=None, lib_path=None, device="cuda:0"):
        self.lib = _capi.load_library(lib_path)
        self.be = backend if backend is not None else TorchCudaBackend(device)
        self.cfg = cfg
        sizes = _capi.GrlSizes()
        check(self.lib, self._query_sizes(cfg, sizes))
        self.sizes = sizes
        self.state = self.be.alloc_f32(sizes.state_bytes)
        self.grads = self.be.alloc_f32(sizes.grads_bytes)
        self.work = self.be.alloc_f32(sizes.work_bytes)
        self.replay = self.be.alloc_f32(sizes.replay_bytes)
        bufs = _capi.GrlBuffers(self.be.ptr(self.state), self.be.ptr(self.grads), self.be.ptr(self.work),
                                self.be.ptr(self.replay))
        h = C.c_void_p()
        check(self.lib, self._create(cfg, bufs, h))
        self.h = h
        check(self.lib, self.lib.grl_set_stream(self.h, C.c_void_p(self.be.stream_ptr())))
        self.table = _capi.param_table(self.lib, self.h)
        self.n_trainable = sizes.n_trainable
        self.B, self.A = cfg.batch_size, cfg.act_dim
        self.observe_rows = int(cfg.act_batch)      # one env step that `observe` + `act(observed=True)` cover in one call
        self._keep = []

    # the two calls that differ between handle kinds (PpoEngine: grl_ppo_query_sizes / grl_ppo_create)
    def _query_sizes(self, cfg, sizes):
        return self.lib.grl_query_sizes(C.byref(cfg), C.byref(sizes))

    def _create(self, cfg, bufs, h):
        return self.lib.grl_create(C.byref(cfg), C.byref(bufs), C.byref(h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.grl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def _view(self, off, numel, shape):
        return self.state[off:off + numel].reshape(shape if len(shape) else ())

    def param_names(self, trainable_only=False):
        return [n for n, _, _, _, tr in self.table if tr or not trainable_only]

    def get_parameters(self):
        """OrderedDict TF-name -> float32 ndarray (SB ``get_parameters``, sb_helper.py:114)."""
        self.be.synchronize()
        out = OrderedDict()
        flat = self.be.to_host(self.state[: self.sizes.n_params])
        for name, off, numel, shape, _ in self.table:
            out[name] = flat[off:off + numel].reshape(shape).copy()
        return out

    def set_parameters(self, params, exact_match=True):
        """SB ``load_parameters(params, exact_match)`` (sb_helper.py:115,198,225)."""
        known = {n for n, *_ in self.table}
        if exact_match and set(params.keys()) != known:
            raise GrlError("parameter names do not match: missing %s, unexpected %s" %
                           (sorted(known - set(params)), sorted(set(params) - known)))
        for name, off, numel, shape, _ in self.table:
            if name not in params:
                continue
            arr = np.asarray(params[name], dtype=np.float32)
            if int(arr.size) != numel:
                raise GrlError("%s: expected shape %s (%d values), got shape %s" % (name, tuple(shape), numel, arr.shape))
            self.be.write(self._view(off, numel, shape), arr.reshape(shape))
        self.be.synchronize()

    def reset_optimizer(self):
        check(self.lib, self.lib.grl_reset_optimizer(self.h))

    def grad_tensor(self):
        """Flat fp32 gradient bucket (the tensor a data-parallel wrapper all-reduces)."""
        return self.grads[: self.n_trainable]

    def get_gradients(self):
        flat = self.be.to_host(self.grads[: self.n_trainable])
        out = OrderedDict()
        for name, off, numel, shape, tr in self.table:
            if tr:
                out[name] = flat[off:off + numel].reshape(shape).copy()
        return out

    # ------------------------------------------------------------------ data
    def set_obs_stats(self, mean, var, ret_var):
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        var = np.ascontiguousarray(var, dtype=np.float64)
        check(self.lib, self.lib.grl_set_obs_stats(self.h, mean.ctypes.data, var.ctypes.data, float(ret_var)))

    # ---- data parallel with the exchange inside the update graph (grl_allreduce_*, csrc/dp_kernels.h)
    HANDLE_BYTES = 128          # include/grl.h: GRL_ALLREDUCE_HANDLE_BYTES (two 64-byte IPC handles: flags, data)

    def allreduce_init(self, rank, world):
        """Allocates this rank's exchange memory; returns its 128 bytes of IPC handles for the out-of-band exchange."""
        buf = C.create_string_buffer(self.HANDLE_BYTES)
        check(self.lib, self.lib.grl_allreduce_init(self.h, int(rank), int(world), buf))
        return buf.raw

    def allreduce_connect(self, handles):
        """handles: the 128-byte handle blobs of all ranks, in rank order."""
        blob = b"".join(handles)
        check(self.lib, self.lib.grl_allreduce_connect(self.h, C.c_char_p(blob)))

    def allreduce_disconnect(self):
        """Back to a single-process handle: peers unmapped, exchange memory freed (grl_allreduce_disconnect).  The caller
        makes sure no exchange is in flight on any rank (DataParallelInGraph.close)."""
        check(self.lib, self.lib.grl_allreduce_disconnect(self.h))

    def allreduce_set_overlap(self, on=True):
        """Exchange the dense bucket on a side lane of the update's graph while the convolution backward runs
        (include/grl.h: grl_allreduce_set_overlap).  Raises when the configuration has no staged plan."""
        check(self.lib, self.lib.grl_allreduce_set_overlap(self.h, 1 if on else 0))

    MODES = {"auto": 0, "twoshot": 1, "oneshot": 2}

    def allreduce_set_mode(self, mode="auto"):
        """'auto' (one-shot for world <= 2), 'twoshot', 'oneshot' (include/grl.h: grl_allreduce_set_mode).  All ranks alike,
        while no exchange is in flight."""
        check(self.lib, self.lib.grl_allreduce_set_mode(self.h, self.MODES[mode]))

    def train_allreduce(self, n_steps=1, idx=None, eps=None):
        pi, pe, keep = self._noise(idx, eps, n_steps)
        check(self.lib, self.lib.grl_train_step_allreduce(self.h, n_steps, pi, pe))
        self._keep = [keep]

    def allreduce_set_timeout(self, ms):
        """Bound of every wait for a peer from now on, in ms (0: the default again); include/grl.h: grl_allreduce_set_timeout."""
        check(self.lib, self.lib.grl_allreduce_set_timeout(self.h, int(ms)))

    def allreduce_status(self):
        n, err = C.c_int64(), C.c_int()
        check(self.lib, self.lib.grl_allreduce_status(self.h, C.byref(n), C.byref(err)))
        return n.value

    # ---- VecNormalize running statistics kept on the device (grl_norm_update; SAC / DQN / BDQ handles)
    def norm_update(self, obs):
        """RunningMeanStd.update(obs) of one env step's raw observations [n, ...] on the device (stream-ordered)."""
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        check(self.lib, self.lib.grl_norm_update(self.h, obs.ctypes.data, obs.shape[0]))

    def observe(self, obs, update_stats=False):
        """Upload one env step's raw observations [n, ...] ONCE (grl_observe): `act(observed=True)` and
        `replay_add_observed` read the device copy; update_stats folds them into the running statistics as `norm_update`
        does.  Returns the serial number of this call (consecutive calls: consecutive numbers)."""
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        check(self.lib, self.lib.grl_observe(self.h, obs.ctypes.data, obs.shape[0], 1 if update_stats else 0))
        self._observe_serial = getattr(self, "_observe_serial", 0) + 1
        return self._observe_serial

    def replay_add_observed(self, act, rew, done, term_rows=None, term_obs=None):
        """The transitions between the last two `observe` calls.  term_rows / term_obs: rows whose episode ended and the
        terminal observations stored as their next observation."""
        rew = np.ascontiguousarray(rew, dtype=np.float32).reshape(-1)
        n = rew.shape[0]
        act = np.ascontiguousarray(act, dtype=np.float32).reshape(n, self.A)
        done = np.ascontiguousarray(done, dtype=np.float32).reshape(n)
        pr = po = None
        n_term = 0
        if term_rows is not None and len(term_rows):
            tr = np.ascontiguousarray(term_rows, dtype=np.int32)
            to = np.ascontiguousarray(term_obs, dtype=np.float32)
            n_term, pr, po = tr.shape[0], tr.ctypes.data, to.ctypes.data
        check(self.lib, self.lib.grl_replay_add_observed(self.h, act.ctypes.data, rew.ctypes.data, done.ctypes.data, n, pr, po, n_term))

    def set_running_stats(self, mean, var, count):
        """Starting point of the running statistics grl_norm_update continues from (env layout, float64)."""
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        var = np.ascontiguousarray(var, dtype=np.float64)
        check(self.lib, self.lib.grl_set_running_stats(self.h, mean.ctypes.data, var.ctypes.data, float(count)))

    def set_ret_var(self, ret_var):
        check(self.lib, self.lib.grl_set_ret_var(self.h, float(ret_var)))

    def get_obs_stats(self, shape):
        """(mean, var, count) of the device statistics, float64, in the observation's shape (synchronises)."""
        mean, var = np.empty(shape, np.float64), np.empty(shape, np.float64)
        cnt = C.c_double()
        check(self.lib, self.lib.grl_get_obs_stats(self.h, mean.ctypes.data, var.ctypes.data, C.byref(cnt)))
        return mean, var, cnt.value

    def set_learning_rate(self, lr):
        check(self.lib, self.lib.grl_set_learning_rate(self.h, float(lr)))

    def replay_add(self, obs, act, rew, next_obs, done):
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (obs, act, rew, next_obs, done)]
        n = arrs[2].reshape(-1).shape[0]
        check(self.lib, self.lib.grl_replay_add(self.h, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data,
                                                arrs[3].ctypes.data, arrs[4].ctypes.data, n))

    def replay_add_device(self, obs, act, rew, next_obs, done):
        """Same with float32 device tensors (already visible to the engine stream)."""
        n = int(rew.numel())
        p = self.be.ptr
        check(self.lib, self.lib.grl_replay_add_device(self.h, p(obs), p(act), p(rew), p(next_obs), p(done), n))

    def replay_size(self):
        return int(self.lib.grl_replay_size(self.h))

    # ------------------------------------------------------------------ checkpoint / resume (DESIGN.md "Checkpoints")
    def replay_segments(self):
        """[(byte offset, bytes per row, rows)] of the replay arena's arrays; rows == 0: an array that is saved whole
        (grl_replay_segments)."""
        segs = (_capi.GrlSegment * 32)()
        n = check(self.lib, self.lib.grl_replay_segments(self.h, 32, segs))
        return [(int(segs[k].offset), int(segs[k].row_bytes), int(segs[k].rows)) for k in range(n)]

    def export_state(self):
        """The handle's host-side state as bytes (grl_state_export; synchronises the stream)."""
        size = C.c_size_t()
        check(self.lib, self.lib.grl_state_size(self.h, C.byref(size)))
        buf = C.create_string_buffer(max(1, size.value))
        n = check(self.lib, self.lib.grl_state_export(self.h, buf, size.value))
        return buf.raw[:n]

    def import_state(self, blob):
        check(self.lib, self.lib.grl_state_import(self.h, C.c_char_p(bytes(blob)), len(blob)))

    def _arena_sizes(self):
        return {k: int(getattr(self.sizes, k)) for k in ("state_bytes", "grads_bytes", "work_bytes", "replay_bytes")}

    @staticmethod
    def _segment_span(seg, filled):
        off, row_bytes, rows = seg
        nbytes = row_bytes * filled if rows else row_bytes
        if off % 4 or nbytes % 4:
            raise GrlError("replay segment is not a whole number of 4-byte words")
        return off // 4, (off + nbytes) // 4

    def save_state(self, dirpath, include_replay=True, extra=None):
        """Writes the full training state of this engine to the directory `dirpath`: meta.json, state.bin (the state arena),
        handle.bin (grl_state_export) and -- unless include_replay is False -- one replay_<k>.bin per array of the replay
        arena, stored rows only.  `extra`: {file name: bytes} written next to them (the model layer's host state), part of
        the same atomic step.  Built as `<dirpath>.tmp`, every file and the directory flushed to the disk, and renamed at
        the end: a save that dies -- or a machine that is reset -- leaves the previous checkpoint as it was, at `dirpath`
        or, between the two renames, at `<dirpath>.old`, where `load_state` finds it.  The page-locked staging buffer is
        released when the save ends."""
        dirpath = os.fspath(dirpath).rstrip("/")
        tmp, old = dirpath + ".tmp", dirpath + ".old"
        if os.path.isdir(tmp):
            shutil.rmtree(tmp)
        os.makedirs(tmp)
        blob = self.export_state()
        hdr = _capi.GrlStateHeader.from_buffer_copy(blob[:C.sizeof(_capi.GrlStateHeader)])
        try:
            return self._save_state(dirpath, tmp, old, blob, hdr, include_replay, extra or {})
        finally:
            _release_staging(self.be)

    def _save_state(self, dirpath, tmp, old, blob, hdr, include_replay, extra):
        for name, raw in [("handle.bin", blob)] + sorted(extra.items()):
            with open(os.path.join(tmp, name), "wb") as f:
                f.write(raw)
                _flush(f)
        with open(os.path.join(tmp, "state.bin"), "wb") as f:
            for chunk in _read_chunks(self.be, self.state, 0, int(self.state.shape[0])):
                f.write(memoryview(chunk).cast("B"))
            _flush(f)
        segs = self.replay_segments()
        if include_replay:
            for k, seg in enumerate(segs):
                lo, hi = self._segment_span(seg, int(hdr.replay_size))
                with open(os.path.join(tmp, "replay_%d.bin" % k), "wb") as f:
                    for chunk in _read_chunks(self.be, self.replay, lo, hi):
                        f.write(memoryview(chunk).cast("B"))
                    _flush(f)
        meta = {"format": CHECKPOINT_FORMAT, "grl_version": int(self.lib.grl_version()),
                "config_hash": "%016x" % hdr.config_hash, "sizes": self._arena_sizes(),
                "state_floats": int(self.state.shape[0]), "handle_bytes": len(blob),
                "segments": [list(sg) for sg in segs], "include_replay": bool(include_replay),
                "replay_size": int(hdr.replay_size), "replay_pos": int(hdr.replay_pos)}
        with open(os.path.join(tmp, "meta.json"), "w") as f:
            json.dump(meta, f, indent=1, sort_keys=True)
            _flush(f)
        _sync_dir(tmp)
        # at every point one complete checkpoint stands at `dirpath` or at `<dirpath>.old`: an `.old` left by a save that
        # died between its renames goes only once `dirpath` exists again
        if os.path.isdir(dirpath):
            if os.path.isdir(old):
                shutil.rmtree(old)
            os.rename(dirpath, old)
        os.rename(tmp, dirpath)
        _sync_dir(os.path.dirname(os.path.abspath(dirpath)))
        if os.path.isdir(old):
            shutil.rmtree(old)
        return meta

    def load_state(self, dirpath):
        """Restores what `save_state` wrote.  Everything is checked before anything changes: format, grl_version(),
        configuration hash, arena sizes, segment table, file sizes and -- by grl_state_import -- the handle blob; a
        mismatch raises GrlError and leaves this engine as it was.  Once those checks have passed the arenas are
        overwritten file by file: an I/O error from then on (a file that changes or becomes unreadable underneath) raises and
        leaves the engine half loaded -- load again or discard it.  A checkpoint saved without its ring restores everything
        else; `replay_size()` is then 0.  The page-locked staging buffer is released when the load ends."""
        try:
            return self._load_state(dirpath)
        finally:
            _release_staging(self.be)

    def _load_state(self, dirpath):
        dirpath = os.fspath(dirpath).rstrip("/")
        if not os.path.isdir(dirpath) and os.path.isdir(dirpath + ".old"):
            dirpath = dirpath + ".old"          # a save died between its two renames: the previous checkpoint
        try:
            with open(os.path.join(dirpath, "meta.json")) as f:
                meta = json.load(f)
        except (OSError, ValueError) as e:
            raise GrlError("no readable checkpoint at %s: %s" % (dirpath, e))
        if meta.get("format") != CHECKPOINT_FORMAT:
            raise GrlError("checkpoint format %r, this build reads %d" % (meta.get("format"), CHECKPOINT_FORMAT))
        if meta.get("grl_version") != int(self.lib.grl_version()):
            raise GrlError("checkpoint written by library version %r, this is %d" % (meta.get("grl_version"), self.lib.grl_version()))
        with open(os.path.join(dirpath, "handle.bin"), "rb") as f:
            blob = f.read()
        hsz = C.sizeof(_capi.GrlStateHeader)
        mine = _capi.GrlStateHeader.from_buffer_copy(self.export_state()[:hsz])
        hdr = _capi.GrlStateHeader.from_buffer_copy(blob[:hsz]) if len(blob) >= hsz else None
        if hdr is None or hdr.magic != _capi.STATE_MAGIC or hdr.config_hash != mine.config_hash:
            # a short or foreign blob, or one of another configuration: grl_state_import refuses it before it changes
            # anything and says why (it names the first grl_config field that differs)
            self.import_state(blob)
            raise GrlError("checkpoint was written for another configuration (config hash)")
        if meta.get("config_hash") != "%016x" % hdr.config_hash:       # the blob is this configuration's: nothing imported
            raise GrlError("meta.json names configuration hash %r, handle.bin %016x" % (meta.get("config_hash"), hdr.config_hash))
        with_ring = bool(meta.get("include_replay"))
        if meta.get("sizes") != self._arena_sizes() or meta.get("state_floats") != int(self.state.shape[0]):
            raise GrlError("checkpoint arena sizes %r differ from this engine's %r" % (meta.get("sizes"), self._arena_sizes()))
        segs = self.replay_segments()
        if [tuple(sg) for sg in meta.get("segments", [])] != segs:
            raise GrlError("checkpoint replay layout differs from this engine's")
        files = [("state.bin", self.state, 0, int(self.state.shape[0]))]
        if with_ring:
            if meta.get("replay_size") != hdr.replay_size or meta.get("replay_pos") != hdr.replay_pos:
                raise GrlError("meta.json and handle.bin disagree about the ring")
            for k, seg in enumerate(segs):
                lo, hi = self._segment_span(seg, int(hdr.replay_size))
                files.append(("replay_%d.bin" % k, self.replay, lo, hi))
        else:                                   # the ring stays out: cursor and size come back as 0
            hdr.replay_pos = hdr.replay_size = 0
            blob = bytes(hdr) + blob[hsz:]
        for name, _, lo, hi in files:
            path = os.path.join(dirpath, name)
            if not os.path.isfile(path) or os.path.getsize(path) != 4 * (hi - lo):
                raise GrlError("checkpoint file %s is missing or has the wrong size" % name)
        self.import_state(blob)                 # the last check (length, layout, host fields); nothing has changed before it
        for name, arena, lo, hi in files:
            with open(os.path.join(dirpath, name), "rb") as f:
                def fill(buf, f=f, name=name):
                    if f.readinto(memoryview(buf).cast("B")) != buf.nbytes:
                        raise GrlError("checkpoint file %s is truncated" % name)
                _write_chunks(self.be, arena, lo, hi, fill)
        # the state arena carries the ring size of the SAVED run (DevScalars.replay_size): importing again lets the blob
        # decide (0 when the ring was left out)
        self.import_state(blob)
        return meta

    # ------------------------------------------------------------------ update
    def _noise(self, idx, eps, n_steps):
        if idx is None and eps is None:
            return None, None, (None, None)
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(n_steps, self.B)
        eps = np.ascontiguousarray(eps, dtype=np.float32).reshape(n_steps, self.B, self.A)
        if idx.min() < 0 or idx.max() >= self.replay_size():
            raise GrlError("replay index out of range")
        di, de = self.be.to_device(idx), self.be.to_device(eps)
        return C.c_void_p(self.be.ptr(di)), C.c_void_p(self.be.ptr(de)), (di, de)

    def train(self, n_steps=1, idx=None, eps=None):
        """n_steps SAC updates; idx/eps (host arrays) make the minibatch and policy noise explicit."""
        pi, pe, keep = self._noise(idx, eps, n_steps)
        check(self.lib, self.lib.grl_train_step(self.h, n_steps, pi, pe))
        self._keep = [keep]   # keep the staged tensors alive until the stream has consumed them

    def train_device(self, n_steps, idx_dev=None, eps_dev=None):
        """Same with idx/eps already resident on the device (or None for the device RNG)."""
        pi = C.c_void_p(self.be.ptr(idx_dev)) if idx_dev is not None else None
        pe = C.c_void_p(self.be.ptr(eps_dev)) if eps_dev is not None else None
        check(self.lib, self.lib.grl_train_step(self.h, n_steps, pi, pe))

    def compute_grads(self, idx=None, eps=None):
        pi, pe, keep = self._noise(idx, eps, 1)
        check(self.lib, self.lib.grl_compute_grads(self.h, pi, pe))
        self._keep = [keep]

    def compute_grads_staged(self, stage, idx=None, eps=None):
        """Stage 0 / 1 of the gradient computation (grl_compute_grads_staged): bucket 0 is final after stage 0."""
        if stage == 0:
            pi, pe, keep = self._noise(idx, eps, 1)
            check(self.lib, self.lib.grl_compute_grads_staged(self.h, 0, pi, pe))
            self._keep = [keep]
        else:
            check(self.lib, self.lib.grl_compute_grads_staged(self.h, 1, None, None))

    def grad_ranges(self, bucket):
        """[(offset, numel)] of gradient bucket 0 (final after stage 0) / 1 (final after stage 1)."""
        offs, nums = (C.c_int64 * 8)(), (C.c_int64 * 8)()
        n = check(self.lib, self.lib.grl_grad_ranges(self.h, bucket, 8, offs, nums))
        return [(int(offs[k]), int(nums[k])) for k in range(n)]

    def apply_grads(self, grad_scale=1.0):
        check(self.lib, self.lib.grl_apply_grads(self.h, float(grad_scale)))

    def metrics(self):
        m = _capi.GrlMetrics()
        check(self.lib, self.lib.grl_get_metrics(self.h, C.byref(m)))
        return {n: getattr(m, n) for n, _ in m._fields_}

    def synchronize(self):
        self.be.synchronize()

    # ------------------------------------------------------------------ sessions: behaviour cloning here (grl_bc_*, csrc/plan_bc.inl), GAIL on TrpoEngine
    def _act_bounds(self, low, high):
        return [np.ascontiguousarray(b, dtype=np.float32).reshape(self.A) for b in (low, high)]

    def _session_open(self, cfg_struct, query_fn, begin_fn):
        nbytes = C.c_size_t()
        check(self.lib, query_fn(self.h, C.byref(cfg_struct), C.byref(nbytes)))
        buf = self.be.alloc_f32(nbytes.value)
        check(self.lib, begin_fn(self.h, C.byref(cfg_struct), C.c_void_p(self.be.ptr(buf))))
        self._session = {"buf": buf, "batch": int(cfg_struct.batch), "keep": None}
        return buf

    def _upload_table(self, obs, act, width):
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        act = np.ascontiguousarray(act, dtype=np.float32).reshape(len(obs), self.A)
        return self.be.to_device(obs.reshape(len(obs), width)), self.be.to_device(act), len(obs)

    def bc_begin(self, batch, learning_rate, adam_epsilon, act_low, act_high):
        """Opens a pretraining session at `batch` rows per minibatch (<= the engine's batch_size): fresh Adam moments and
        beta powers, its own buffer.  act_low / act_high: the action space's bounds."""
        low, high = self._act_bounds(act_low, act_high)
        c = _capi.GrlBcConfig(int(batch), float(learning_rate), float(adam_epsilon), low.ctypes.data, high.ctypes.data)
        self._session_open(c, self.lib.grl_bc_query_sizes, self.lib.grl_bc_begin)

    def bc_upload(self, obs, act):
        """(observations, actions) of a dataset as float32 device arrays for bc_train / bc_eval: [n, obs_size], [n, A]."""
        return self._upload_table(obs, act, -1)

    def _bc_call(self, fn, table, idx):
        obs, act, n = table
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, self._session["batch"])
        di = self.be.to_device(idx)
        p = self.be.ptr
        check(self.lib, fn(self.h, p(obs), p(act), n, C.c_void_p(p(di)), idx.shape[0]))
        self._session["keep"] = (table, di)      # alive until the stream has consumed them

    def bc_train(self, table, idx):
        """One update per row of idx [n_updates, batch] (int32 rows of the table; a shorter minibatch ends in -1 entries),
        back to back on the stream.  table: what bc_upload returned."""
        self._bc_call(self.lib.grl_bc_train, table, idx)

    def bc_eval(self, table, idx):
        """Forward and loss only over the rows of idx [n_batches, batch]."""
        self._bc_call(self.lib.grl_bc_eval, table, idx)

    def bc_losses(self):
        """Per-update / per-batch losses of the last bc_train / bc_eval call (synchronises)."""
        out = np.empty(_capi.BC_MAX_UPDATES, np.float32)
        n = check(self.lib, self.lib.grl_bc_get_losses(self.h, out.ctypes.data, out.size))
        return out[:n].copy()

    def bc_end(self):
        check(self.lib, self.lib.grl_bc_end(self.h))
        self._session = None

    # ------------------------------------------------------------------ inference
    def act(self, obs, deterministic=True, eps=None, raw=False, observed=False):
        """raw=True: `obs` are un-normalised observations, VecNormalize is applied on the device (norm_update statistics).
        observed=True: act on the observations the last `observe` uploaded (`obs` is then only looked at for its length)."""
        if observed:
            n, po = int(obs if np.isscalar(obs) else len(obs)), None
        else:
            obs = np.ascontiguousarray(obs, dtype=np.float32)
            n, po = obs.shape[0], obs.ctypes.data
        out = np.empty((n, self.A), np.float32)
        pe = None
        if not deterministic:
            eps = np.ascontiguousarray(eps, dtype=np.float32).reshape(n, self.A)
            pe = eps.ctypes.data
        flags = (1 if deterministic else 0) | (2 if raw else 0) | (4 if observed else 0)
        check(self.lib, self.lib.grl_act(self.h, po, n, flags, pe, out.ctypes.data))
        return out

    def load_encoder(self, weights):
        """weights: Keras order conv2d_1..3 kernel/bias, dense_1 kernel/bias (encoders.py:90-108)."""
        arrs = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        ptrs = (C.c_void_p * 8)(*[a.ctypes.data for a in arrs])
        nums = (C.c_int64 * 8)(*[a.size for a in arrs])
        check(self.lib, self.lib.grl_encoder_load(self.h, ptrs, nums, 8))

    encoding_dim = 100       # floats per image `encode` returns (auto-encoder handles: their configured encoding_dim)

    def encode(self, depth):
        depth = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1, 64, 64, 1)
        n = depth.shape[0]
        out = np.empty((n, self.encoding_dim), np.float32)
        check(self.lib, self.lib.grl_encode(self.h, depth.ctypes.data, n, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ debugging / profiling
    def fetch(self, name, shape=None):
        cap = 1 << 24
        buf = np.empty(cap, np.float32) if shape is None else np.empty(int(np.prod(shape)), np.float32)
        n = check(self.lib, self.lib.grl_debug_fetch(self.h, name.encode(), buf.ctypes.data, buf.size))
        out = buf[:n].copy()
        return out.reshape(shape) if shape is not None else out

    def store(self, name, arr):
        """Overwrite a named internal tensor (parity tests only; grl_debug_store)."""
        arr = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        check(self.lib, self.lib.grl_debug_store(self.h, name.encode(), arr.ctypes.data, arr.size))

    def profile(self, on):
        check(self.lib, self.lib.grl_profile_enable(self.h, 1 if on else 0))

    def profile_dump(self):
        buf = C.create_string_buffer(1 << 14)
        check(self.lib, self.lib.grl_profile_dump(self.h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            tag, ms, n, fl, by, fx = line.split(":")
            out[tag] = {"avg_ms": float(ms), "launches": int(n), "flops": float(fl), "bytes": float(by),
                        "flops_executed": float(fx)}
        return out


class Td3Engine(SacEngine):
    """TD3 handle (``_capi.make_td3_config``): arenas, replay ring, statistics calls, parameters, ``set_learning_rate``,
    ``reset_optimizer`` (both Adams), ``fetch`` / ``store`` and profiling as on a SAC handle on vector observations; ``train``
    runs twin-critic updates with the delayed policy update, ``act`` returns pi(obs)."""

    METRIC_NAMES = ("qf1_loss", "qf2_loss", "policy_loss", "mean_q1", "mean_q2", "policy_updated")

    def __init__(self, cfg, td3, backend=None, lib_path=None, device="cuda:0"):
        self.td3 = td3
        super().__init__(cfg, backend=backend, lib_path=lib_path, device=device)
        self.obs_dim = cfg.obs_dim
        self.ldq = (cfg.obs_dim + cfg.act_dim + 3) // 4 * 4      # row stride of the critics' input rows ("td3_xs", "td3_xn")

    def _query_sizes(self, cfg, sizes):
        return self.lib.grl_td3_query_sizes(C.byref(cfg), C.byref(self.td3), C.byref(sizes))

    def _create(self, cfg, bufs, h):
        return self.lib.grl_td3_create(C.byref(cfg), C.byref(self.td3), C.byref(bufs), C.byref(h))

    def train(self, n_updates=1, idx=None, eps=None, first_step=0):
        """n_updates updates in one call; update u is a policy update iff (first_step + u) % policy_delay == 0.  idx
        [n_updates, B] replay rows / eps [n_updates, B, A] standard normals of the target smoothing (host arrays): either may be
        None for device draws."""
        di = de = None
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(n_updates, self.B)
            if idx.min() < 0 or idx.max() >= self.replay_size():
                raise GrlError("replay index out of range")
            di = self.be.to_device(idx)
        if eps is not None:
            de = self.be.to_device(np.ascontiguousarray(eps, dtype=np.float32).reshape(n_updates, self.B, self.A))
        pi = C.c_void_p(self.be.ptr(di)) if di is not None else None
        pe = C.c_void_p(self.be.ptr(de)) if de is not None else None
        check(self.lib, self.lib.grl_td3_train(self.h, int(n_updates), pi, pe, int(first_step)))
        self._keep = [(di, de)]   # keep the staged tensors alive until the stream has consumed them

    def metrics(self):
        """[n_updates, 6] of the last ``train``: columns METRIC_NAMES (synchronises)."""
        out = np.empty((_capi.TD3_MAX_UPDATES, _capi.TD3_METRICS), np.float32)
        n = check(self.lib, self.lib.grl_td3_get_metrics(self.h, out.ctypes.data, out.size))
        return out[:n].copy()

    def act(self, obs, deterministic=True, eps=None, raw=False, observed=False):
        """pi(obs) of n <= act_batch observations (exploration noise is the caller's: `deterministic` and `eps` change nothing).
        raw=True: un-normalised observations, VecNormalize applied on the device."""
        if observed:
            raise GrlError("TD3: observe / act(observed=True) is not implemented")
        obs = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1, self.obs_dim)
        out = np.empty((obs.shape[0], self.A), np.float32)
        check(self.lib, self.lib.grl_act(self.h, obs.ctypes.data, obs.shape[0], 1 | (2 if raw else 0), None, out.ctypes.data))
        return out

    def adam_steps(self):
        """(critic steps, policy steps) the two Adams have taken, from their beta1 powers."""
        return tuple(int(round(np.log(float(self.fetch(n, (2,))[0])) / np.log(0.9))) - 1 for n in ("td3_beta_c", "td3_beta_pi"))


class QEngine(SacEngine):
    """DQN / BDQ handle (``_capi.make_q_config``): same arenas and calls -- ``norm_update``, ``set_running_stats``,
    ``get_obs_stats``, ``observe`` / ``observe_rows`` and ``replay_add_observed`` (action columns: the bins [n, branches]) as
    on a SAC handle; the explicit-noise slot of ``train`` / ``compute_grads`` carries prioritised-replay importance weights
    [n_steps, B] and ``act`` returns dueling Q-values [n, branches, bins]."""

    def __init__(self, cfg, backend=None, lib_path=None, device="cuda:0"):
        super().__init__(cfg, backend=backend, lib_path=lib_path, device=device)
        self.D, self.bins = cfg.q_branches, cfg.q_bins

    def _noise(self, idx, weights, n_steps):
        if idx is None and weights is None:
            return None, None, (None, None)
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(n_steps, self.B)
        if weights is None:
            weights = np.ones((n_steps, self.B), np.float32)
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(n_steps, self.B)
        if idx.min() < 0 or idx.max() >= self.replay_size():
            raise GrlError("replay index out of range")
        di, dw = self.be.to_device(idx), self.be.to_device(weights)
        return C.c_void_p(self.be.ptr(di)), C.c_void_p(self.be.ptr(dw)), (di, dw)

    def q_values(self, obs):
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        n = obs.shape[0]
        out = np.empty((n, self.D * self.bins), np.float32)
        check(self.lib, self.lib.grl_act(self.h, obs.ctypes.data, n, 1, None, out.ctypes.data))
        return out.reshape(n, self.D, self.bins)

    def act(self, obs, deterministic=True, eps=None):
        return self.q_values(obs).argmax(axis=2)

    def act_bins(self, obs, explore=None, raw=False, observed=False):
        """Epsilon-greedy bins [n, branches] (int64) of n <= act_batch observations: the arg-max of the dueling Q-values per
        branch, formed on the device (grl_act with GRL_ACT_GREEDY; one launch, csrc/q_act.h).  explore [n, branches]: an
        entry >= 0 replaces the greedy bin of that (row, branch), a negative one keeps it; None = all greedy.  The caller
        draws the randomness.  raw=True: `obs` are un-normalised observations, VecNormalize is applied on the device
        (norm_update statistics).  observed=True: act on the observations the last `observe` uploaded (`obs` is then only
        looked at for its length)."""
        if observed:
            n, po = int(obs if np.isscalar(obs) else len(obs)), None
        else:
            obs = np.ascontiguousarray(obs, dtype=np.float32)
            n, po = obs.shape[0], obs.ctypes.data
        out = np.empty((n, self.D), np.float32)
        pe = None
        if explore is not None:
            explore = np.ascontiguousarray(explore, dtype=np.float32).reshape(n, self.D)
            pe = explore.ctypes.data
        flags = _capi.ACT_GREEDY | (2 if raw else 0) | (4 if observed else 0)
        check(self.lib, self.lib.grl_act(self.h, po, n, flags, pe, out.ctypes.data))
        return out.astype(np.int64)

    def update_target(self):
        check(self.lib, self.lib.grl_q_update_target(self.h))

    # ---- prioritised replay on the device (cfg.q_per; csrc/per_kernels.h)
    def train_per(self, n_steps=1, beta=1.0, u=None):
        """n_steps updates on minibatches drawn proportionally to the stored priority**alpha leaves, with importance
        weights (N p)^-beta / max; the leaves of the trained transitions are refreshed on the device afterwards
        (stable-baselines PrioritizedReplayBuffer.sample / update_priorities).
        u: optional host array [n_steps, B] of float64 uniforms in [0, 1) (parity tests); None = device RNG."""
        pu, keep = None, None
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64).reshape(n_steps, self.B)
            keep = self.be.to_device(u)
            pu = C.c_void_p(self.be.ptr(keep))
        check(self.lib, self.lib.grl_train_step_per(self.h, n_steps, float(beta), pu))
        self._keep = [keep]

    def sampled_indices(self):
        return self.fetch("idx_raw", (2 * self.B,)).view(np.int64).copy()

    def importance_weights(self):
        return self.fetch("weights", (self.B,))

    def stored_priorities(self):
        """float64 leaves priority**alpha of every slot of the ring (zeros where nothing is stored)"""
        return self.fetch("per_p", (2 * int(self.cfg.replay_capacity),)).view(np.float64).copy()

    def store_priorities(self, leaves):
        """Overwrite the float64 leaves (parity tests only)."""
        self.store("per_p", np.ascontiguousarray(leaves, np.float64).view(np.float32))

    def td_errors(self):
        return self.fetch("td", (self.B, self.D))

    def priorities(self):
        return self.fetch("priority", (self.B,))


class PpoEngine(SacEngine):
    """PPO2 handle (``_capi.make_ppo_config``): the rollout lives on the device; ``step`` / ``rewards`` fill a slot per env step,
    ``finish`` forms the last values and GAE, ``train`` runs noptepochs * nminibatches updates over the permutations handed to
    it.  Parameters, ``set_learning_rate``, ``reset_optimizer``, ``fetch`` / ``store`` and profiling as on every handle.

    A handle configured with ``normalize=2`` keeps VecNormalize's observation statistics: ``observe`` (the n_envs raw rows of one
    env step, one upload and one launch), ``set_obs_stats`` / ``set_running_stats`` / ``get_obs_stats`` are SacEngine's methods,
    and ``step`` / ``finish`` with ``obs=None`` act on the rows the last ``observe`` normalised."""

    def __init__(self, cfg, ppo, backend=None, lib_path=None, device="cuda:0"):
        self.ppo = ppo
        super().__init__(cfg, backend=backend, lib_path=lib_path, device=device)
        self.n_envs, self.n_steps, self.obs_dim = ppo.n_envs, ppo.n_steps, cfg.obs_dim
        self.R = self.n_envs * self.n_steps
        self.ldo = (self.obs_dim + 3) // 4 * 4
        self.n_minibatches = self.R // cfg.batch_size
        self.observe_rows = self.n_envs      # grl_observe on these handles takes exactly one env step of all environments

    def _query_sizes(self, cfg, sizes):
        return self.lib.grl_ppo_query_sizes(C.byref(cfg), C.byref(self.ppo), C.byref(sizes))

    def _create(self, cfg, bufs, h):
        return self.lib.grl_ppo_create(C.byref(cfg), C.byref(self.ppo), C.byref(bufs), C.byref(h))

    def step(self, obs, done, eps=None):
        """model.step on the n_envs observations: (actions [n, A] unclipped, values [n], neglogps [n]); recorded in the open slot.
        obs None: the rows the last ``observe`` normalised on the device."""
        n, A = self.n_envs, self.A
        if obs is not None:
            obs = np.ascontiguousarray(obs, dtype=np.float32).reshape(n, self.obs_dim)
        done = np.ascontiguousarray(done, dtype=np.float32).reshape(n)
        pe = None
        if eps is not None:
            eps = np.ascontiguousarray(eps, dtype=np.float32).reshape(n, A)
            pe = eps.ctypes.data
        act, val, nlp = np.empty((n, A), np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
        check(self.lib, self.lib.grl_ppo_step(self.h, None if obs is None else obs.ctypes.data, done.ctypes.data, pe, act.ctypes.data, val.ctypes.data,
                                              nlp.ctypes.data))
        return act, val, nlp

    def rewards(self, rew):
        rew = np.ascontiguousarray(rew, dtype=np.float32).reshape(self.n_envs)
        check(self.lib, self.lib.grl_ppo_rewards(self.h, rew.ctypes.data, self.n_envs))

    def finish(self, last_obs, last_done):
        if last_obs is not None:      # (None: the rows the last ``observe`` normalised)
            last_obs = np.ascontiguousarray(last_obs, dtype=np.float32).reshape(self.n_envs, self.obs_dim)
        last_done = np.ascontiguousarray(last_done, dtype=np.float32).reshape(self.n_envs)
        check(self.lib, self.lib.grl_ppo_finish(self.h, None if last_obs is None else last_obs.ctypes.data, last_done.ctypes.data))

    def train(self, perm):
        """perm [noptepochs, R] int32: one permutation of the rollout rows per epoch."""
        perm = np.ascontiguousarray(perm, dtype=np.int32).reshape(-1, self.R)
        check(self.lib, self.lib.grl_ppo_train(self.h, perm.ctypes.data, perm.shape[0]))

    def metrics(self):
        """[n_updates, 5] of the last ``train``: policy loss, value loss, entropy, approxkl, clipfrac."""
        out = np.empty((_capi.PPO_MAX_EPOCHS * max(1, self.n_minibatches), 5), np.float32)
        n = check(self.lib, self.lib.grl_ppo_get_metrics(self.h, out.ctypes.data, out.size))
        return out[:n].copy()

    def act(self, obs, deterministic=True, eps=None):
        """model.predict-style action (unclipped) of n <= n_envs observations; eps None with deterministic=False: device draw."""
        obs = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1, self.obs_dim)
        n = obs.shape[0]
        out = np.empty((n, self.A), np.float32)
        pe = None
        if not deterministic and eps is not None:
            eps = np.ascontiguousarray(eps, dtype=np.float32).reshape(n, self.A)
            pe = eps.ctypes.data
        check(self.lib, self.lib.grl_act(self.h, obs.ctypes.data, n, 1 if deterministic else 0, pe, out.ctypes.data))
        return out

    def reset_rollout(self):
        """Empty the rollout (slot 0 is next), whatever state a stopped run left it in."""
        self.store("ppo_slots", [0, 0, 0])

    # ------------------------------------------------------------------ checkpoint / resume
    # save_state / load_state are SacEngine's: same directory protocol, meta.json, state.bin, handle.bin and extra files.  What
    # differs is the blob (grl_ppo_state_*) and the replay arena, which holds the rollout and is written whole as replay_0.bin.
    def export_state(self):
        """The handle's host-side state as bytes (grl_ppo_state_export; synchronises the stream): the rollout cursor, the parity
        of the statistics' double buffer and the rows the last ``observe`` normalised."""
        size = C.c_size_t()
        check(self.lib, self.lib.grl_ppo_state_size(self.h, C.byref(size)))
        buf = C.create_string_buffer(max(1, size.value))
        n = check(self.lib, self.lib.grl_ppo_state_export(self.h, buf, size.value))
        return buf.raw[:n]

    def import_state(self, blob):
        check(self.lib, self.lib.grl_ppo_state_import(self.h, C.c_char_p(bytes(blob)), len(blob)))

    def replay_segments(self):
        """One array saved whole: the rollout arena of R = n_envs * n_steps rows (no ring, no stored-rows prefix;
        grl_replay_segments stays undefined on these handles)."""
        return [(0, 4 * int(self.replay.shape[0]), 0)]

    def rollout_cursor(self):
        """(slots written, slots closed, finished) as grl_ppo_state_export reports them."""
        blob = self.export_state()
        second = C.sizeof(self.trpo) if hasattr(self, "trpo") else C.sizeof(self.ppo)
        off = C.sizeof(_capi.GrlStateHeader) + C.sizeof(_capi.GrlConfig) + second
        written, closed, finished = np.frombuffer(blob, np.int32, 3, off)
        return int(written), int(closed), bool(finished)

    def _load_state(self, dirpath):
        meta = super()._load_state(dirpath)
        if not meta.get("include_replay"):      # the rollout stayed out: an empty one (cursor 0 / 0 / not finished)
            self.reset_rollout()
        return meta

    def place_rollout(self, obs, act, val, nlp, rew, done):
        """Parity tests: a whole rollout through grl_debug_store.  Arrays are [n_envs, n_steps, ...] (row = env * n_steps + t)."""
        o = np.zeros((self.R, self.ldo), np.float32)
        o[:, :self.obs_dim] = np.asarray(obs, np.float32).reshape(self.R, self.obs_dim)
        for name, arr in (("ppo_obs", o), ("ppo_act", act), ("ppo_old_v", val), ("ppo_old_nlp", nlp), ("ppo_rew", rew),
                          ("ppo_done", done)):
            self.store(name, arr)
        self.store("ppo_slots", [self.n_steps, self.n_steps, 0])


class TrpoEngine(PpoEngine):
    """TRPO handle (``_capi.make_trpo_config``): the rollout calls are PpoEngine's with one environment (``done`` is the step's
    episode_start; ``finish`` forms V(last observation), GAE and tdlamret); ``update`` runs the natural-gradient policy step and
    the value fit of one learn iteration on the device."""

    METRIC_NAMES = ("optimgain", "meankl", "entbonus", "surrgain", "meanent", "ls_index", "trial_optimgain", "trial_meankl",
                    "cg_iters", "rr", "shs")

    def __init__(self, cfg, trpo, backend=None, lib_path=None, device="cuda:0"):
        self.trpo = trpo
        ppo = _capi.GrlPpoConfig()      # (what PpoEngine reads: one environment of n_steps rows)
        ppo.n_envs, ppo.n_steps = 1, trpo.n_steps
        super().__init__(cfg, ppo, backend=backend, lib_path=lib_path, device=device)
        self.T, self.vf_batch = trpo.n_steps, trpo.vf_batch
        self.n_minibatches = self.T // self.vf_batch

    def _query_sizes(self, cfg, sizes):
        return self.lib.grl_trpo_query_sizes(C.byref(cfg), C.byref(self.trpo), C.byref(sizes))

    def _create(self, cfg, bufs, h):
        return self.lib.grl_trpo_create(C.byref(cfg), C.byref(self.trpo), C.byref(bufs), C.byref(h))

    def train(self, perm):
        raise GrlError("a TRPO handle updates with update(vf_perm)")

    def update(self, vf_perm=None):
        """vf_perm [vf_iters, T] int32, each row a permutation of the rollout rows (None: no value fit)."""
        if vf_perm is None or len(vf_perm) == 0:
            check(self.lib, self.lib.grl_trpo_update(self.h, None, 0))
            return
        vf_perm = np.ascontiguousarray(vf_perm, dtype=np.int32).reshape(-1, self.T)
        check(self.lib, self.lib.grl_trpo_update(self.h, vf_perm.ctypes.data, vf_perm.shape[0]))

    def metrics(self):
        """The last update: dict of METRIC_NAMES (ls_index: accepted trial, -1 restored, -2 zero gradient)."""
        out = np.empty(_capi.TRPO_METRICS, np.float32)
        check(self.lib, self.lib.grl_trpo_get_metrics(self.h, out.ctypes.data, out.size))
        m = {k: float(v) for k, v in zip(self.METRIC_NAMES, out)}
        m["ls_index"], m["cg_iters"] = int(m["ls_index"]), int(m["cg_iters"])
        return m

    def fisher_vector_product(self, vec):
        """Parity: F(vec) at the current parameters over the Fisher rows of the full rollout on the device; vec and the result
        are laid out like the gradient bucket ([n_trainable]).  The entries of the value variables are ignored: they are
        cleared here, since the engine expects them zero, and come back zero."""
        vec = np.array(vec, np.float32).reshape(-1)
        for name, off, numel, _, trainable in self.table:
            if trainable and "/pi" not in name:
                vec[off:off + numel] = 0.0
        self.store("trpo_fvp_in", vec)
        check(self.lib, self.lib.grl_trpo_debug_fvp(self.h))
        return self.fetch("trpo_fvp_out", (int(self.sizes.n_trainable),))

    # ------------------------------------------------------------------ GAIL (grl_gail_*, csrc/plan_gail.inl)
    LOSS_NAMES = ("generator_loss", "expert_loss", "entropy", "entropy_loss", "generator_acc", "expert_acc")

    def gail_begin(self, hidden, batch, entcoeff, learning_rate, act_low, act_high, adam_epsilon=1e-8, params=None):
        """Opens a GAIL session: a discriminator of two tanh layers of `hidden` units, `batch` generator rows per update, its own
        Adam and running statistics, in a buffer of its own.  The parameters start at zero: hand them as `params` (name ->
        array, the six ``adversary/...`` tensors) or store them with ``gail_set_parameters``."""
        low, high = self._act_bounds(act_low, act_high)
        c = _capi.GrlGailConfig(int(hidden), int(batch), float(entcoeff), float(learning_rate), float(adam_epsilon), low.ctypes.data, high.ctypes.data)
        self._session_open(c, self.lib.grl_gail_query_sizes, self.lib.grl_gail_begin)
        table = self._session["table"] = []
        for i in range(6):
            name = C.create_string_buffer(128)
            off, numel, rows, cols = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
            check(self.lib, self.lib.grl_gail_param_info(self.h, i, name, 128, C.byref(off), C.byref(numel), C.byref(rows), C.byref(cols)))
            shape = (rows.value, cols.value) if i % 2 == 0 else (rows.value,)
            table.append((name.value.decode(), off.value, numel.value, shape))
        if params is not None:
            self.gail_set_parameters(params)

    def gail_param_shapes(self):
        return OrderedDict((name, shape) for name, _, _, shape in self._session["table"])

    def _gail_block(self, name):
        n = max(off + numel for _, off, numel, _ in self._session["table"])
        return self.fetch(name, ((n + 3) // 4 * 4,))

    def gail_get_parameters(self, block="gail_params"):
        """name -> array of the six tensors (block: "gail_params", "gail_adam_m", "gail_adam_v" or "gail_grads")."""
        flat = self._gail_block(block)
        return OrderedDict((name, flat[off:off + numel].reshape(shape).copy()) for name, off, numel, shape in self._session["table"])

    def gail_set_parameters(self, params):
        flat = self._gail_block("gail_params")
        for name, off, numel, shape in self._session["table"]:
            flat[off:off + numel] = np.asarray(params[name], np.float32).reshape(-1)
        self.store("gail_params", flat)

    def gail_upload(self, obs, act):
        """(observations, actions) of an expert dataset as float32 device arrays for gail_update: [n, obs_dim], [n, A]."""
        return self._upload_table(obs, act, self.obs_dim)

    def gail_rewards(self):
        """Rewrites the rewards of the full, not yet finished rollout with the discriminator's (one batched pass)."""
        check(self.lib, self.lib.grl_gail_rewards(self.h))

    def gail_update(self, table, gen_idx, exp_idx):
        """One discriminator update per row of gen_idx / exp_idx [n_updates, batch] (int32: rows of the last finished rollout;
        rows of the table, a shorter expert batch ending in -1 entries).  table: what gail_upload returned."""
        obs, act, n = table
        b = self._session["batch"]
        gi = np.ascontiguousarray(gen_idx, dtype=np.int32).reshape(-1, b)
        ei = np.ascontiguousarray(exp_idx, dtype=np.int32).reshape(-1, b)
        if gi.shape != ei.shape:
            raise GrlError("gail_update: gen_idx and exp_idx must name the same number of updates")
        dg, de = self.be.to_device(gi), self.be.to_device(ei)
        p = self.be.ptr
        self._session["keep"] = (table, dg, de)      # alive until the stream has consumed them
        check(self.lib, self.lib.grl_gail_update(self.h, p(obs), p(act), n, C.c_void_p(p(dg)), C.c_void_p(p(de)), gi.shape[0]))

    def gail_losses(self):
        """[n_updates, 6] of the last gail_update, columns LOSS_NAMES (synchronises)."""
        out = np.empty((_capi.GAIL_MAX_UPDATES, 6), np.float32)
        n = check(self.lib, self.lib.grl_gail_get_losses(self.h, out.ctypes.data, out.size))
        return out[:n].copy()

    def gail_get_stats(self):
        """(sum [obs_dim], sumsq [obs_dim], count) of the discriminator's input statistics, float64."""
        s, q, c = np.empty(self.obs_dim, np.float64), np.empty(self.obs_dim, np.float64), C.c_double()
        check(self.lib, self.lib.grl_gail_get_stats(self.h, s.ctypes.data, q.ctypes.data, C.byref(c)))
        return s, q, c.value

    def gail_set_stats(self, total, sumsq, count):
        s = np.ascontiguousarray(total, dtype=np.float64).reshape(self.obs_dim)
        q = np.ascontiguousarray(sumsq, dtype=np.float64).reshape(self.obs_dim)
        check(self.lib, self.lib.grl_gail_set_stats(self.h, s.ctypes.data, q.ctypes.data, float(count)))

    def gail_end(self):
        check(self.lib, self.lib.grl_gail_end(self.h))
        self._session = None
